// engine_proof.cpp -- Explain with proofs (include/aclgpu.h acl_explain_proof*): Check + hops + absences for items that a permission with `-`, `&` or `.all()`
// beneath grants (Snapshot::slot_nonmono).  Items of monotone slots go through explain_walk (engine_explain.cpp) and come back as acl_explain_bulk_ids returns them.
//
// A proof is searched over GOALS: derive state (object, slot) for the item's subject within d dispatches, or refute an expression of a subtracted operand.
// The Schema's rewrite tree (the one plan.cpp compiles the combine programs from) says what a goal needs; the relationship store, which an Eval holds at the
// snapshot's revision, says which rows there are; and every choice -- which member of a row to step to, which operand of a union holds, whether a subtracted
// operand is absent -- is made by the device: the members of a row become candidate items there (k_proof_items), check_device answers them and k_proof_pick
// folds the answers per goal, so that 28 bytes per goal come back whatever the row's length.  A row that is only stepped through (a relation's userset row,
// the tupleset row of an arrow that is derived) is enumerated by the device as well (k_proof_rows, into a region that is redone larger when it overflows);
// a row whose members all end up in the proof (an arrow under an exclusion, `.all()`) is read from the store.  A goal on a MONOTONE slot that a Check has
// granted is not searched at all: explain_walk walks the whole positive stretch beneath it in one block of k_explain_local and traces the chain back on the
// device, so the rounds of a proof follow its combine states, not its dispatches (derive_state, chain_depth).  A stand-alone Check is more permissive about depth than the
// same state inside a proof, and a state already on the path proves nothing new: a confirmed candidate whose own proof fails is dropped and the next one that
// answered HAS is asked for.  The search of one item is a plain recursion that runs against the answers known so far; where it needs one that is not known it
// notes the question and gives up, the questions of all items of the batch go to the device as one pass, and the unfinished items run again.  So the device
// sees one pass per round of the deepest proof, not one per goal; a round's searches run on the host's threads.
#include <unordered_map>
#include <unordered_set>

#include "engine_internal.hpp"
#include "validate.hpp"

namespace aclint {

namespace {

constexpr uint32_t kProofMaxGoals = 1u << 20;      // states one run of one item's search may open: beyond, ACL_ERR_RESOURCE_EXHAUSTED
constexpr size_t kProofPassCands = (size_t)1 << 22;  // host-made candidates of one device pass, at most (whole groups; one group may be longer)
constexpr size_t kProofPassGroups = (size_t)1 << 16;  // ... and its groups
constexpr uint32_t kProofRegionFirst = 1u << 14, kProofRegionMax = 1u << 24;  // ids of the rows one pass enumerates on the device: first attempt, at most
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr int kMaxDispatch = 50;                   // pkg/spicedb/spicedb.go:34

enum R : int { R_NO = 0, R_YES = 1, R_NEED = 2 };  // R_NEED: an answer the search depends on is not known yet (the question is in the round's list)

struct QKey {       // one question: candidates [floor, end) of one class of one row, asked on behalf of one state or one arrow node
    uint64_t a, b;  // a: the arrow's Node, or slot | kind << 60;  b: object | class index << 32
    uint32_t floor;
    bool operator==(const QKey &o) const { return a == o.a && b == o.b && floor == o.floor; }
};
struct QHash {
    size_t operator()(const QKey &k) const {
        uint64_t x = k.a * 0x9E3779B97F4A7C15ull ^ (k.b + 0x7F4A7C15ull) * 0xC2B2AE3D27D4EB4Full ^ (uint64_t)k.floor * 0x165667B19E3779F9ull;
        return (size_t)(x ^ x >> 29);
    }
};
struct QRes {  // k_proof_pick's fold of the answers: indices inside [floor, end), and the two candidates they name (k_proof_winner)
    uint32_t first_has, first_no, n_has, n_no, n, has_obj, no_obj;
};
struct RowRef {  // where the device keeps the sorted sub-rows of one (relation, subject class): descriptor base + object * K + k (plan.hpp FwdOp)
    uint32_t base, K, k, nrows;
};
using RowRefs = std::unordered_map<uint64_t, RowRef>;  // slot << 16 | class index
using Cache = std::unordered_map<QKey, QRes, QHash>;
struct Pending {
    uint32_t prover;
    QKey key;
    uint32_t head, tail, sid;
    std::vector<uint32_t> objs;  // the candidates, enumerated by the host ...
    uint32_t meta_idx = kNone;   // ... or the descriptor of the row the device enumerates itself from `floor` on (k_proof_rows): they never cross PCIe
};

struct WalkReq {  // one monotone state whose witness chain k_explain_local is to find (explain_walk)
    uint32_t prover;
    uint64_t key;  // slot << 32 | object
    acl_item_t item;
};

struct Prover {
    acl_engine *h;
    const Schema &sc;
    int64_t now;
    uint32_t self;  // index among the call's provers
    size_t index;   // the item's index in the batch
    acl_item_t it;
    int st, srel;
    uint32_t sid, tail;
    Cache cache;
    std::unordered_set<QKey, QHash> asked;
    std::vector<Pending> *pending;
    const RowRefs *rowrefs;
    std::vector<WalkReq> *walks_pending;
    std::unordered_map<uint64_t, std::vector<acl_explain_hop_t>> walks;  // the chains found so far, by state
    std::unordered_set<uint64_t> walk_asked, walk_too_deep;            // too deep: the chain does not fit the dispatches left where the state is needed
    std::vector<acl_explain_hop_t> hops;
    std::vector<acl_item_t> absent;
    std::vector<uint64_t> path;  // derive goals on the stack: slot << 32 | object
    uint32_t goals = 0;
    int stop = 0;  // 1: kProofMaxGoals, 2: ACL_PROOF_MAX_RECORDS
    // what this round's run asked for, and how it ended: the searches of a round run on the host's threads, each into its own lists
    std::vector<Pending> my_pend;
    std::vector<WalkReq> my_walks;
    R last = R_NEED;

    Prover(acl_engine *h_, int64_t now_, uint32_t self_, size_t index_, const acl_item_t &it_, const RowRefs *rr)
        : h(h_), sc(h_->store.schema()), now(now_), self(self_), index(index_), it(it_), pending(&my_pend), rowrefs(rr), walks_pending(&my_walks) {
        st = it.subject_type;
        srel = it.subject_relation == ACL_NO_RELATION ? kNoRelation : (int)it.subject_relation;
        sid = it.subject_id;
        tail = (uint32_t)it.subject_type | (uint32_t)it.subject_relation << 16;
    }

    struct Mark {
        size_t nh, na;
    };
    Mark mark() const { return Mark{hops.size(), absent.size()}; }
    void rollback(const Mark &m) {
        hops.resize(m.nh);
        absent.resize(m.na);
    }
    bool room(size_t more) {
        if (hops.size() + absent.size() + more > ACL_PROOF_MAX_RECORDS) stop = 2;
        return !stop;
    }
    void hop(int t, int m, uint32_t o, const SubjectClass &c, uint32_t s) {
        if (!room(1)) return;
        hops.push_back(acl_explain_hop_t{(uint16_t)t, (uint16_t)m, o, (uint16_t)c.stype, (uint16_t)(c.srel == kNoRelation ? ACL_NO_RELATION : c.srel), s,
                                         c.wildcard ? ACL_HOP_WILDCARD : 0u});
    }
    void absence(int t, int m, uint32_t o) {
        if (!room(1)) return;
        absent.push_back(acl_item_t{(uint16_t)t, (uint16_t)m, o, it.subject_type, it.subject_relation, sid});
    }

    // the live subjects of row (slot, class, object), ascending
    std::vector<uint32_t> row(int slot, size_t ci, uint32_t o) const {
        std::vector<uint32_t> out;
        const ClassTable &ct = h->store.tables()[slot][ci];
        const uint64_t lo = (uint64_t)o << 32;
        for (auto k = std::lower_bound(ct.keys.begin(), ct.keys.end(), lo); k != ct.keys.end() && (*k >> 32) == o; ++k)
            if (h->store.live(ct, *k, now)) out.push_back((uint32_t)*k);
        return out;
    }
    bool row_has(int slot, size_t ci, uint32_t o, uint32_t s) const {
        const ClassTable &ct = h->store.tables()[slot][ci];
        const uint64_t key = (uint64_t)o << 32 | s;
        return std::binary_search(ct.keys.begin(), ct.keys.end(), key) && h->store.live(ct, key, now);
    }

    // the device's fold over objs[floor ..) as Check items (type t, member m, the item's subject); nullptr: not known yet, asked for
    const QRes *ask(const QKey &k, int t, int m, const std::vector<uint32_t> &objs) {
        auto f = cache.find(k);
        if (f != cache.end()) return &f->second;
        if (k.floor >= objs.size()) return &cache.emplace(k, QRes{kNone, kNone, 0, 0, 0, kNone, kNone}).first->second;
        if (asked.insert(k).second)
            pending->push_back(Pending{self, k, (uint32_t)t | (uint32_t)m << 16, tail, sid, std::vector<uint32_t>(objs.begin() + k.floor, objs.end()), kNone});
        return nullptr;
    }
    // the same over the members of object o's row from k.floor on, which the device enumerates
    const QRes *ask_row(const QKey &k, int t, int m, const RowRef &rr, uint32_t o) {
        auto f = cache.find(k);
        if (f != cache.end()) return &f->second;
        if (o >= rr.nrows) return &cache.emplace(k, QRes{kNone, kNone, 0, 0, 0, kNone, kNone}).first->second;
        if (asked.insert(k).second)
            pending->push_back(Pending{self, k, (uint32_t)t | (uint32_t)m << 16, tail, sid, std::vector<uint32_t>(), rr.base + o * rr.K + rr.k});
        return nullptr;
    }
    const QRes *ask_one(int t, int m, uint32_t o) { return ask(QKey{(uint64_t)sc.slot(t, m) | 1ull << 60, o, 0}, t, m, std::vector<uint32_t>{o}); }

    // steps from a row's class to one of its members: the first candidate that answered HAS and whose own proof succeeds
    template <typename Emit, typename Next>
    R step(QKey k, int ct, int cm, int slot, size_t ci, uint32_t o, Emit emit, Next next) {
        const auto rr = rowrefs->find((uint64_t)slot << 16 | ci);
        if (rr != rowrefs->end()) {  // the row stays on the device: only the chosen member comes back
            for (uint32_t floor = 0;;) {
                k.floor = floor;
                const QRes *q = ask_row(k, ct, cm, rr->second, o);
                if (!q) return R_NEED;
                if (q->first_has == kNone || q->has_obj == kNone) return R_NO;
                const Mark mk = mark();
                emit(q->has_obj);
                const R r = next(q->has_obj);
                if (r == R_YES) return R_YES;
                rollback(mk);
                if (r == R_NEED || stop) return r;
                if (q->first_has + 1u >= q->n) return R_NO;
                floor += q->first_has + 1u;
            }
        }
        const std::vector<uint32_t> members = row(slot, ci, o);
        for (uint32_t floor = 0; floor < members.size();) {
            k.floor = floor;
            const QRes *q = ask(k, ct, cm, members);
            if (!q) return R_NEED;
            if (q->first_has == kNone) return R_NO;
            const uint32_t i = floor + q->first_has;
            if (i >= members.size()) return R_NO;
            const Mark mk = mark();
            emit(members[i]);
            const R r = next(members[i]);
            if (r == R_YES) return R_YES;
            rollback(mk);
            if (r == R_NEED || stop) return r;
            floor = i + 1;
        }
        return R_NO;
    }

    R derive_state(int t, int m, uint32_t o, int d) {
        if (stop || d <= 0) return R_NO;
        if (t == st && m == srel && o == sid) return R_YES;
        if (++goals > kProofMaxGoals) {
            stop = 1;
            return R_NO;
        }
        const uint64_t pk = (uint64_t)sc.slot(t, m) << 32 | o;
        if (std::find(path.begin(), path.end(), pk) != path.end()) return R_NO;  // (a proof that passes through its own goal holds a shorter one)
        const Member &mem = sc.defs[t].members[m];
        const size_t slot = pk >> 32;
        if (!(slot < h->snap.slot_nonmono.size() && h->snap.slot_nonmono[slot]) && !walk_too_deep.count(pk)) {
            // a monotone state: the whole positive stretch beneath it is ONE walk of k_explain_local -- parents in its log, the chain traced back on
            // the device -- however many dispatches it spans.  The walk is asked for only once a Check has granted the state on its own (the walk of
            // a state that is not granted is Explain's "the two kernels disagree").
            if (!mem.is_permission && direct_hit(t, m, o)) return stop ? R_NO : R_YES;  // (one look at the store: no device round)
            const QRes *q = ask_one(t, m, o);
            if (!q) return R_NEED;
            if (q->n_has != 1) return R_NO;
            auto wf = walks.find(pk);
            if (wf == walks.end()) {
                if (walk_asked.insert(pk).second) walks_pending->push_back(WalkReq{self, pk, acl_item_t{(uint16_t)t, (uint16_t)m, o, it.subject_type, it.subject_relation, sid}});
                return R_NEED;
            }
            // the walk had the full 50 dispatches; here d are left: the chain counts only if it fits (else the state is searched a dispatch at a time)
            if (chain_depth(t, m, o, wf->second, 0) <= d) {
                if (!room(wf->second.size())) return R_NO;
                hops.insert(hops.end(), wf->second.begin(), wf->second.end());
                return R_YES;
            }
            walk_too_deep.insert(pk);
        }
        path.push_back(pk);
        const R r = mem.is_permission ? derive(mem.expr, t, o, d) : derive_relation(t, m, o, d);
        path.pop_back();
        return r;
    }

    // the least number of dispatches within which state (t, m, o) derives from the relationships of chain `w` alone (a monotone state: unions, references,
    // arrows and relations), counted as derive_state counts them; kTooDeep: it does not
    static constexpr int kTooDeep = 1000;
    int chain_depth(int t, int m, uint32_t o, const std::vector<acl_explain_hop_t> &w, int rec) const {
        if (t == st && m == srel && o == sid) return 1;
        if (rec > 64) return kTooDeep;
        const Member &mem = sc.defs[t].members[m];
        if (!mem.is_permission) {
            int best = kTooDeep;
            for (const acl_explain_hop_t &x : w) {
                if (x.rtype != t || x.relation != m || x.rid != o) continue;
                if (x.stype == it.subject_type && x.srel == it.subject_relation && (x.sid == sid || (x.flags & ACL_HOP_WILDCARD))) return 1;
                if (x.srel != ACL_NO_RELATION) best = std::min(best, 1 + chain_depth(x.stype, x.srel, x.sid, w, rec + 1));
            }
            return best;
        }
        return expr_depth(mem.expr, t, o, w, rec);
    }
    int expr_depth(const Node &e, int t, uint32_t o, const std::vector<acl_explain_hop_t> &w, int rec) const {
        int best = kTooDeep;
        if (e.kind == Node::kUnion) {
            for (const Node &k : e.kids) best = std::min(best, expr_depth(k, t, o, w, rec));
        } else if (e.kind == Node::kRef) {
            const int m = sc.defs[t].find(e.a);
            if (m >= 0) best = 1 + chain_depth(t, m, o, w, rec + 1);
        } else if (e.kind == Node::kArrow) {
            const int tm = sc.defs[t].find(e.a);
            for (const acl_explain_hop_t &x : w) {
                if (tm < 0 || x.rtype != t || x.relation != tm || x.rid != o || (x.flags & ACL_HOP_WILDCARD)) continue;
                const int pm = sc.defs[x.stype].find(e.b);
                if (pm >= 0) best = std::min(best, 1 + chain_depth(x.stype, pm, x.sid, w, rec + 1));
            }
        }
        return best;
    }

    // relation m of o names the subject itself, or its type's `*`: that hop
    bool direct_hit(int t, int m, uint32_t o) {
        const Member &mem = sc.defs[t].members[m];
        const int slot = sc.slot(t, m);
        for (size_t ci = 0; ci < mem.classes.size(); ci++) {
            const SubjectClass &c = mem.classes[ci];
            if (c.stype != st || c.srel != srel) continue;
            const uint32_t s = c.wildcard ? h->store.wildcard_id(st) : sid;
            if (s != kNone && row_has(slot, ci, o, s)) {
                hop(t, m, o, c, s);
                return true;
            }
        }
        return false;
    }

    R derive_relation(int t, int m, uint32_t o, int d) {
        const Member &mem = sc.defs[t].members[m];
        const int slot = sc.slot(t, m);
        if (direct_hit(t, m, o)) return stop ? R_NO : R_YES;
        R out = R_NO;
        for (size_t ci = 0; ci < mem.classes.size(); ci++) {  // a userset hop o#m@x#s whose state (x, s) derives, one dispatch down
            const SubjectClass &c = mem.classes[ci];
            if (c.srel == kNoRelation) continue;
            const R r = step(QKey{(uint64_t)slot | 2ull << 60, (uint64_t)o | (uint64_t)ci << 32, 0}, c.stype, c.srel, slot, ci, o,
                             [&](uint32_t x) { hop(t, m, o, c, x); }, [&](uint32_t x) { return derive_state(c.stype, c.srel, x, d - 1); });
            if (r == R_YES) return R_YES;
            if (r == R_NEED) out = R_NEED;
            if (stop) return R_NO;
        }
        return out;
    }

    template <typename F>
    R any_of(size_t n, F f) {
        R out = R_NO;
        for (size_t k = 0; k < n && !stop; k++) {
            const Mark mk = mark();
            const R r = f(k);
            if (r == R_YES) return R_YES;
            rollback(mk);
            if (r == R_NEED) out = R_NEED;
        }
        return stop ? R_NO : out;
    }
    template <typename F>
    R all_of(size_t n, F f) {
        const Mark mk = mark();
        R out = R_YES;
        for (size_t k = 0; k < n; k++) {
            const R r = f(k);
            if (r == R_NO || stop) {
                rollback(mk);
                return R_NO;
            }
            if (r == R_NEED) out = R_NEED;  // (the other operands' questions join this round's)
        }
        return out;
    }

    // the classes of tupleset relation tm of type t whose subject type has member `name`: fn(class index, class, member index there)
    template <typename F>
    void arrow_classes(int t, int tm, const std::string &name, F fn) const {
        const Member &ts = sc.defs[t].members[tm];
        for (size_t ci = 0; ci < ts.classes.size(); ci++) {
            const SubjectClass &c = ts.classes[ci];
            const int pm = c.wildcard ? -1 : sc.defs[c.stype].find(name);
            if (pm >= 0) fn(ci, c, pm);
        }
    }

    R derive(const Node &e, int t, uint32_t o, int d) {
        if (stop) return R_NO;
        switch (e.kind) {
        case Node::kNil: return R_NO;
        case Node::kUnion: return any_of(e.kids.size(), [&](size_t k) { return derive(e.kids[k], t, o, d); });
        case Node::kIntersect: return all_of(e.kids.size(), [&](size_t k) { return derive(e.kids[k], t, o, d); });
        case Node::kExclude: return all_of(2, [&](size_t k) { return k == 0 ? derive(e.kids[0], t, o, d) : refute(e.kids[1], t, o, d); });
        case Node::kRef: {
            const int m = sc.defs[t].find(e.a);
            if (m < 0) return R_NO;
            if (sc.defs[t].members[m].is_permission) {  // (a relation's row decides on the host; a permission is worth one question before its proof is tried)
                const QRes *q = ask_one(t, m, o);
                if (!q) return R_NEED;
                if (q->n_has != 1) return R_NO;
            }
            return derive_state(t, m, o, d - 1);
        }
        case Node::kArrow: {
            const int tm = sc.defs[t].find(e.a);
            if (tm < 0) return R_NO;
            const int slot = sc.slot(t, tm);
            R out = R_NO;
            bool done = false;
            arrow_classes(t, tm, e.b, [&](size_t ci, const SubjectClass &c, int pm) {
                if (done || stop) return;
                const R r = step(QKey{(uint64_t)(uintptr_t)&e | 3ull << 60, (uint64_t)o | (uint64_t)ci << 32, 0}, c.stype, pm, slot, ci, o, [&](uint32_t x) { hop(t, tm, o, c, x); },
                                 [&](uint32_t x) { return derive_state(c.stype, pm, x, d - 1); });
                if (r == R_YES) out = R_YES, done = true;
                else if (r == R_NEED) out = R_NEED;
            });
            return stop ? R_NO : out;
        }
        case Node::kArrowAll: {
            const int tm = sc.defs[t].find(e.a);
            if (tm < 0) return R_NO;
            const int slot = sc.slot(t, tm);
            size_t total = 0;
            R out = R_YES;
            arrow_classes(t, tm, e.b, [&](size_t ci, const SubjectClass &c, int pm) {  // every member answers HAS on its own, or there is nothing to prove
                if (out == R_NO) return;
                const std::vector<uint32_t> members = row(slot, ci, o);
                total += members.size();
                if (members.empty() || !room(total)) return;
                const QRes *q = ask(QKey{(uint64_t)(uintptr_t)&e, (uint64_t)o | (uint64_t)ci << 32, 0}, c.stype, pm, members);
                if (!q) out = R_NEED;
                else if (q->n_has != members.size()) out = R_NO;
            });
            if (!total || out != R_YES || stop) return (!total || stop) ? R_NO : out;
            const Mark mk = mark();
            arrow_classes(t, tm, e.b, [&](size_t ci, const SubjectClass &c, int pm) {
                if (out == R_NO) return;
                for (uint32_t x : row(slot, ci, o)) {
                    hop(t, tm, o, c, x);
                    const R r = derive_state(c.stype, pm, x, d - 1);
                    if (r == R_NO || stop) {
                        out = R_NO;
                        return;
                    }
                    if (r == R_NEED) out = R_NEED;
                }
            });
            if (out == R_NO) rollback(mk);
            return out;
        }
        }
        return R_NO;
    }

    // the subtracted operand e does not hold: by absences (and the tupleset hops that lead to them), or by a proof of what IT subtracts
    R refute(const Node &e, int t, uint32_t o, int d) {
        if (stop) return R_NO;
        switch (e.kind) {
        case Node::kNil: return R_YES;
        case Node::kUnion: return all_of(e.kids.size(), [&](size_t k) { return refute(e.kids[k], t, o, d); });
        case Node::kIntersect: return any_of(e.kids.size(), [&](size_t k) { return refute(e.kids[k], t, o, d); });
        case Node::kExclude: return any_of(2, [&](size_t k) { return k == 0 ? refute(e.kids[0], t, o, d) : derive(e.kids[1], t, o, d); });
        case Node::kRef: {
            const int m = sc.defs[t].find(e.a);
            if (m < 0) return R_YES;
            const QRes *q = ask_one(t, m, o);
            if (!q) return R_NEED;
            if (q->n_no != 1) return R_NO;
            absence(t, m, o);
            return stop ? R_NO : R_YES;
        }
        case Node::kArrow: {  // every member of the tupleset row is absent
            const int tm = sc.defs[t].find(e.a);
            if (tm < 0) return R_YES;
            const int slot = sc.slot(t, tm);
            size_t total = 0;
            R out = R_YES;
            arrow_classes(t, tm, e.b, [&](size_t ci, const SubjectClass &c, int pm) {
                if (out == R_NO) return;
                const std::vector<uint32_t> members = row(slot, ci, o);
                total += members.size();
                if (members.empty() || !room(2 * total)) return;
                const QRes *q = ask(QKey{(uint64_t)(uintptr_t)&e, (uint64_t)o | (uint64_t)ci << 32, 0}, c.stype, pm, members);
                if (!q) out = R_NEED;
                else if (q->n_no != members.size()) out = R_NO;
            });
            if (stop) return R_NO;
            if (out != R_YES) return out;
            arrow_classes(t, tm, e.b, [&](size_t ci, const SubjectClass &c, int pm) {
                for (uint32_t x : row(slot, ci, o)) {
                    hop(t, tm, o, c, x);
                    absence(c.stype, pm, x);
                }
            });
            return stop ? R_NO : R_YES;
        }
        case Node::kArrowAll: {  // no member at all, or one that is absent
            const int tm = sc.defs[t].find(e.a);
            if (tm < 0) return R_YES;
            const int slot = sc.slot(t, tm);
            size_t total = 0;
            R out = R_NO;
            arrow_classes(t, tm, e.b, [&](size_t ci, const SubjectClass &c, int pm) {
                if (out == R_YES) return;
                const std::vector<uint32_t> members = row(slot, ci, o);
                total += members.size();
                if (members.empty()) return;
                const QRes *q = ask(QKey{(uint64_t)(uintptr_t)&e, (uint64_t)o | (uint64_t)ci << 32, 0}, c.stype, pm, members);
                if (!q) {
                    out = R_NEED;
                } else if (q->first_no != kNone && q->first_no < members.size()) {
                    hop(t, tm, o, c, members[q->first_no]);
                    absence(c.stype, pm, members[q->first_no]);
                    out = R_YES;
                }
            });
            if (stop) return R_NO;
            return total ? out : R_YES;
        }
        }
        return R_NO;
    }

    // one run against the answers known so far
    R run() {
        hops.clear();
        absent.clear();
        path.clear();
        goals = 0;
        return derive_state(it.resource_type, it.permission, it.resource_id, kMaxDispatch);
    }
};

// one device pass over the questions pend[p0, p1): candidates (the host's, then the rows the device enumerates into a region of *region ids behind them)
// -> items -> Check -> per-group fold; the answers go into the askers' caches.  A row that outgrows the region redoes the pass with one 8 times as large
int proof_pass(acl_engine *h, PassCtx *c, std::vector<std::unique_ptr<Prover>> &provers, const std::vector<Pending> &pend, size_t p0, size_t p1, uint32_t *region) {
    const size_t ng = p1 - p0;
    size_t nhost = 0, ndev = 0;
    for (size_t g = p0; g < p1; g++) {
        nhost += pend[g].objs.size();
        ndev += pend[g].meta_idx != kNone;
    }
    if (nhost >= 0x7FFFFFFFull) return fail(ACL_ERR_RESOURCE_EXHAUSTED, "Explain proof: more than 2^31 candidates in one pass");
    const DevState &d = *c->dev;
    for (;;) {
        const size_t cap = nhost + (ndev ? *region : 0);
        HIP_TRY(c->d_proof_obj.ensure(cap));
        HIP_TRY(c->d_proof_group.ensure(cap));
        HIP_TRY(c->d_proof_groups.ensure(ng));
        HIP_TRY(c->d_proof_rows.ensure(2 * ng));
        HIP_TRY(c->d_proof_out.ensure(4 + 7 * ng));  // total[3] (+ pad) | first[2 ng] | count[2 ng] | win[2 ng] | gn[ng]
        HIP_TRY(c->h_in.ensure(nhost * 8 + ng * (sizeof(uint4) + sizeof(uint2)) + 16));
        HIP_TRY(c->h_out.ensure((4 + 7 * ng) * sizeof(uint32_t) + 64));
        uint4 *hg = (uint4 *)c->h_in.p;  // (16-byte aligned: the headers first)
        uint2 *hr = (uint2 *)(hg + ng);
        uint32_t *ht = (uint32_t *)(hr + ng), *ho = ht + 4, *hgr = ho + nhost;
        size_t at = 0;
        for (size_t g = 0; g < ng; g++) {
            const Pending &p = pend[p0 + g];
            hg[g] = make_uint4(p.head, p.tail, p.sid, (uint32_t)at);
            hr[g] = make_uint2(p.meta_idx, p.key.floor);
            if (p.meta_idx != kNone) continue;
            std::memcpy(ho + at, p.objs.data(), p.objs.size() * sizeof(uint32_t));
            std::fill(hgr + at, hgr + at + p.objs.size(), (uint32_t)g);
            at += p.objs.size();
        }
        ht[0] = (uint32_t)nhost, ht[1] = 0, ht[2] = 0, ht[3] = 0;
        uint32_t *d_total = c->d_proof_out.p, *d_first = d_total + 4, *d_count = d_first + 2 * ng, *d_win = d_count + 2 * ng, *d_gn = d_win + 2 * ng;
        HIP_TRY(hipMemcpyAsync(c->d_proof_groups.p, hg, ng * sizeof(uint4), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->d_proof_rows.p, hr, ng * sizeof(uint2), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_total, ht, 4 * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        if (nhost) {
            HIP_TRY(hipMemcpyAsync(c->d_proof_obj.p, ho, nhost * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(c->d_proof_group.p, hgr, nhost * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        }
        HIP_TRY(hipMemsetAsync(d_first, 0xFF, 2 * ng * sizeof(uint32_t), c->stream));
        HIP_TRY(hipMemsetAsync(d_count, 0, 2 * ng * sizeof(uint32_t), c->stream));
        HIP_TRY(hipMemsetAsync(d_gn, 0, ng * sizeof(uint32_t), c->stream));
        size_t ncand = nhost;
        if (ndev) {
            const DevProofRows rw{d.d_meta.p, d.d_edges.p, (uint32_t)(h->snap.meta.size() / 2), (uint32_t)h->snap.edges.size(), (const uint2 *)c->d_proof_rows.p,
                                  c->d_proof_groups.p, d_gn, c->d_proof_obj.p, c->d_proof_group.p, (uint32_t)cap, (uint32_t)ng, d_total};
            ev_begin(c, 0);
            launch_proof_rows(c->stream, rw);
            ev_end(c);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(c->h_out.p, d_total, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            ev_collect(c);
            const uint32_t *t = (const uint32_t *)c->h_out.p;
            if (t[2] || t[1] || t[0] > cap) {  // a row did not fit
                c->stats.overflow_retries++;
                if (*region >= kProofRegionMax) return fail(ACL_ERR_RESOURCE_EXHAUSTED, "Explain proof: the rows of one pass outgrew their region (2^24 candidates)");
                *region = std::min(*region * 8u, kProofRegionMax);
                continue;
            }
            ncand = t[0];
        }
        const DevProofPick pk{c->d_proof_obj.p, c->d_proof_group.p, c->d_proof_groups.p, (uint32_t)ncand, (uint32_t)ng, d_first, d_count};
        if (ncand) {
            HIP_TRY(c->d_items.ensure(ncand));
            HIP_TRY(c->d_perm.ensure(ncand));
            HIP_TRY(c->d_errout.ensure(ncand));
            ev_begin(c, 0);
            launch_proof_items(c->stream, pk, c->d_items.p);
            ev_end(c);
            HIP_TRY(hipGetLastError());
            int rc = check_device(h, c, c->d_items.p, ncand, c->d_perm.p, c->d_errout.p);  // (ends with the stream synchronised)
            if (rc) return rc;
            ev_begin(c, 0);
            launch_proof_pick(c->stream, pk, c->d_perm.p, c->d_errout.p, ACL_PERM_HAS_PERMISSION, ACL_PERM_NO_PERMISSION);
            ev_end(c);
        }
        ev_begin(c, 0);
        launch_proof_winner(c->stream, pk, d_win);
        ev_end(c);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c->h_out.p, c->d_proof_out.p, (4 + 7 * ng) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        ev_collect(c);
        const uint32_t *first = (const uint32_t *)c->h_out.p + 4, *count = first + 2 * ng, *win = count + 2 * ng, *gn = win + 2 * ng;
        for (size_t g = 0; g < ng; g++) {
            const Pending &p = pend[p0 + g];
            const uint32_t n = p.meta_idx != kNone ? gn[g] : (uint32_t)p.objs.size();
            provers[p.prover]->cache[p.key] = QRes{first[2 * g], first[2 * g + 1], count[2 * g], count[2 * g + 1], n, win[2 * g], win[2 * g + 1]};
        }
        return ACL_OK;
    }
}

// caller holds an Eval with the subject rows current
int proof_batch(acl_engine *h, PassCtx *c, const acl_item_t *items, size_t n, uint8_t *perm, int32_t *err, uint8_t *flags, uint32_t *hop_off, acl_explain_hop_t **hops_out,
                uint32_t *absent_off, acl_item_t **absent_out) {
    const Schema &sc = h->store.schema();
    int rc = check_ids_chunked(h, c, items, n, perm, err);
    if (rc) return rc;
    std::vector<uint32_t> mono;
    std::vector<Pending> pend;
    std::vector<std::unique_ptr<Prover>> provers;
    // the sorted sub-rows the device can enumerate itself: whatever class an enumerating op of some program reads (the side table names it)
    RowRefs rowrefs;
    if (h->subj.xops.size() != h->snap.ops.size()) return fail(ACL_ERR_INTERNAL, "Explain proof: the per-op side table does not match the programs");
    for (size_t j = 0; j < h->snap.ops.size(); j++) {
        const FwdOp &op = h->snap.ops[j];
        const ExplainOp &x = h->subj.xops[j];
        if (!(op.flags & OP_ENUM) || (op.flags & (OP_PROBE_HASH | OP_PUSH_SAME | OP_REFLEX)) || x.rtype == ExplainOp::kExplainRewrite) continue;
        if (x.rtype >= sc.defs.size() || x.relation >= sc.defs[x.rtype].members.size()) continue;
        const std::vector<SubjectClass> &cls = sc.defs[x.rtype].members[x.relation].classes;
        for (size_t ci = 0; ci < cls.size(); ci++)
            if (!cls[ci].wildcard && cls[ci].stype == x.stype && (uint16_t)(cls[ci].srel == kNoRelation ? 0xFFFF : cls[ci].srel) == x.srel)
                rowrefs.emplace((uint64_t)sc.slot(x.rtype, x.relation) << 16 | ci, RowRef{op.base, op.K, op.k, op.nrows});
    }
    std::vector<WalkReq> walkreqs;
    // the rows the host reads are read at ONE time, inside the window the snapshot was built for: host and device see the same relationships live
    int64_t now = h->store.now();
    if (h->snap.valid_hi > h->snap.valid_lo) now = std::min(std::max(now, h->snap.valid_lo), h->snap.valid_hi - 1);
    uint32_t &region = c->proof_region;  // (kept across calls: a graph whose rows outgrew the first region once does not pay the redo again)
    if (region < kProofRegionFirst) region = kProofRegionFirst;
    rc = explain_classify(h, "Explain proof", ACL_PERM_HAS_PERMISSION, items, n, perm, err, flags, [&](size_t i, const acl_item_t &it, uint32_t, bool nonmono) {
        if (nonmono) provers.emplace_back(new Prover(h, now, (uint32_t)provers.size(), i, it, &rowrefs));
        else mono.push_back((uint32_t)i);
    });
    if (rc) return rc;
    std::vector<acl_explain_hop_t> mhops;
    std::vector<uint32_t> mcount;
    rc = explain_walk(h, c, items, mono, &mhops, &mcount);
    if (rc) return rc;
    // rounds: every unfinished search runs against what is known, then one device pass (or a few, by size) answers what they asked
    std::vector<uint32_t> active(provers.size());
    for (size_t k = 0; k < active.size(); k++) active[k] = (uint32_t)k;
    while (!active.empty()) {
        rc = check_opts(c->opts);
        if (rc) return rc;
        pend.clear();
        walkreqs.clear();
        std::vector<uint32_t> still;
        // (the searches read the store and the snapshot, which the Eval holds still, and write only their own state)
        host_parallel(h, active.size(), 64, [&](size_t b, size_t e) {
            for (size_t k = b; k < e; k++) {
                Prover &p = *provers[active[k]];
                p.my_pend.clear();
                p.my_walks.clear();
                p.last = p.run();
            }
        });
        for (uint32_t k : active) {
            Prover &p = *provers[k];
            const R r = p.last;
            for (Pending &q : p.my_pend) pend.push_back(std::move(q));
            walkreqs.insert(walkreqs.end(), p.my_walks.begin(), p.my_walks.end());
            if (p.stop == 1)
                return fail(ACL_ERR_RESOURCE_EXHAUSTED, "Explain proof: the search for " + explain_item_text(p.it, p.index) + " opened more than 2^20 goals");
            if (p.stop == 2)
                return fail(ACL_ERR_RESOURCE_EXHAUSTED, "Explain proof: the proof of " + explain_item_text(p.it, p.index) + " holds more than " +
                                                            std::to_string(ACL_PROOF_MAX_RECORDS) + " hops and absences");
            if (r == R_NO)
                return fail(ACL_ERR_INTERNAL, "Explain proof: Check grants " + explain_item_text(p.it, p.index) + " but no proof was found within the depth limit");
            if (r == R_NEED) {
                still.push_back(k);
            } else {  // done: the answers are not needed any more
                Cache().swap(p.cache);
                std::unordered_set<QKey, QHash>().swap(p.asked);
            }
        }
        if (!still.empty() && pend.empty() && walkreqs.empty()) return fail(ACL_ERR_INTERNAL, "Explain proof: a search waits for an answer nobody asked for");
        for (size_t p0 = 0; p0 < pend.size();) {
            size_t p1 = p0, nc = 0;
            for (; p1 < pend.size() && (p1 == p0 || (nc + pend[p1].objs.size() <= kProofPassCands && p1 - p0 < kProofPassGroups)); p1++) nc += pend[p1].objs.size();
            rc = proof_pass(h, c, provers, pend, p0, p1, &region);
            if (rc) return rc;
            p0 = p1;
        }
        if (!walkreqs.empty()) {  // the round's monotone stretches: one launch of k_explain_local for all of them (per chunk), a block each
            std::vector<acl_item_t> witems(walkreqs.size());
            std::vector<uint32_t> wpick(walkreqs.size()), wcount;
            std::vector<acl_explain_hop_t> whops;
            for (size_t k = 0; k < walkreqs.size(); k++) witems[k] = walkreqs[k].item, wpick[k] = (uint32_t)k;
            rc = explain_walk(h, c, witems.data(), wpick, &whops, &wcount);
            if (rc) return rc;
            size_t at = 0;
            for (size_t k = 0; k < walkreqs.size(); k++) {
                provers[walkreqs[k].prover]->walks[walkreqs[k].key].assign(whops.begin() + at, whops.begin() + at + wcount[k]);
                at += wcount[k];
            }
        }
        active.swap(still);
    }
    std::fill(hop_off, hop_off + n + 1, 0u);
    std::fill(absent_off, absent_off + n + 1, 0u);
    size_t nh = mhops.size(), na = 0;
    for (size_t k = 0; k < mono.size(); k++) {
        flags[mono[k]] = ACL_EXPLAIN_WITNESS;
        hop_off[mono[k] + 1] = mcount[k];
    }
    for (const auto &p : provers) {
        flags[p->index] = ACL_EXPLAIN_PROOF;
        hop_off[p->index + 1] = (uint32_t)p->hops.size();
        absent_off[p->index + 1] = (uint32_t)p->absent.size();
        nh += p->hops.size();
        na += p->absent.size();
    }
    if (nh >= 0xFFFFFFFFull || na >= 0xFFFFFFFFull) return fail(ACL_ERR_RESOURCE_EXHAUSTED, "Explain proof: more than 2^32 records in one call");
    for (size_t i = 0; i < n; i++) hop_off[i + 1] += hop_off[i], absent_off[i + 1] += absent_off[i];
    acl_explain_hop_t *out = nullptr;
    acl_item_t *aout = nullptr;
    rc = result_block(nh, "out of host memory for the proofs", &out);
    if (!rc) rc = result_block(na, "out of host memory for the proofs", &aout);
    if (rc) {
        std::free(out);  // (the hops' block is the only one that can be held here)
        return rc;
    }
    size_t mh = 0;
    for (size_t k = 0; k < mono.size(); k++) {  // (explain_walk appends in pick order)
        if (mcount[k]) std::memcpy(out + hop_off[mono[k]], mhops.data() + mh, mcount[k] * sizeof(acl_explain_hop_t));
        mh += mcount[k];
    }
    for (const auto &p : provers) {
        acl_explain_hop_t *dst = out + hop_off[p->index];
        for (size_t k = 0; k < p->hops.size(); k++) {
            dst[k] = p->hops[k];
            // a hop that does not continue the one before it starts a new chain
            if (k && (dst[k].rtype != dst[k - 1].stype || dst[k].rid != dst[k - 1].sid || (dst[k - 1].flags & ACL_HOP_WILDCARD))) dst[k].flags |= ACL_HOP_SEGMENT;
        }
        if (!p->absent.empty()) std::memcpy(aout + absent_off[p->index], p->absent.data(), p->absent.size() * sizeof(acl_item_t));
    }
    *hops_out = out;
    *absent_out = aout;
    return ACL_OK;
}

}  // namespace

}  // namespace aclint

int acl_explain_proof_bulk_ids(acl_engine_t *h, const acl_item_t *items, size_t n, uint8_t *perm_out, int32_t *err_out, uint8_t *flags_out, uint32_t *hop_off_out,
                               acl_explain_hop_t **hops_out, uint32_t *absent_off_out, acl_item_t **absent_out, const acl_call_opts_t *opts) {
    return explain_front(
        h, "acl_explain_proof_bulk_ids", items, n, perm_out, err_out, flags_out, opts,
        [&](PassCtx *c, int32_t *err, uint8_t *flags) { return proof_batch(h, c, items, n, perm_out, err, flags, hop_off_out, hops_out, absent_off_out, absent_out); },
        ExplainOut<acl_explain_hop_t>{hop_off_out, hops_out}, ExplainOut<acl_item_t>{absent_off_out, absent_out});
}

int acl_explain_proof(acl_engine_t *h, const acl_check_item_t *item, uint8_t *perm_out, int32_t *err_out, uint32_t *flags_out, char **text_out, const acl_call_opts_t *opts) {
    return explain_one_front(
        h, "acl_explain_proof", "out of host memory for the proof", item, perm_out, err_out, flags_out, text_out, [&](const acl_item_t &it, uint8_t *flag, std::string *text) {
            uint8_t fl = 0;
            uint32_t off[2] = {0, 0}, aoff[2] = {0, 0};
            acl_explain_hop_t *hops = nullptr;
            acl_item_t *absent = nullptr;
            int rc = acl_explain_proof_bulk_ids(h, &it, 1, perm_out, err_out, &fl, off, &hops, aoff, &absent, opts);
            if (rc) return rc;
            *flag = fl;
            rc = explain_hops_text(h, "acl_explain_proof", hops, off[0], off[1], text);
            // an absence names its goal as a hop names a relationship: the object, the relation or permission, the item's subject
            for (uint32_t k = aoff[0]; k < aoff[1] && !rc; k++) {
                const acl_explain_hop_t goal{absent[k].resource_type, absent[k].permission, absent[k].resource_id, absent[k].subject_type, absent[k].subject_relation,
                                             absent[k].subject_id, 0u};
                *text += "not ";
                rc = explain_hops_text(h, "acl_explain_proof", &goal, 0, 1, text);
            }
            std::free(hops);
            std::free(absent);
            return rc;
        });
}

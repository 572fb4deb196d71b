// engine_denial.cpp -- Explain for denials (include/aclgpu.h acl_explain_denial*): Check + every single relationship whose write would grant a denied item.
//
// A Check of R#P@S that answers NO without error on a monotone permission has looked at a closed set of states (object, relation or permission): the forward
// closure of R#P over userset and arrow relationships.  S is in none of their rows, so the relationships `o#r@S` with (o, r) in that closure and r accepting
// S's class are exactly the single writes that turn the answer into HAS.  One Eval holds the call: the batch is answered by the ordinary Check
// (check_ids_host), the denied items are grouped by (resource type, resource id, permission), and k_reach_local (kernels.hip) walks each group's closure
// once, one block each -- the walk does not depend on the subject.  The device returns STATES; which relationships they stand for is read off the SCHEMA
// here (denial_grants), not off the programs' ops: the programs hold no op for a class without a live relationship, and a relation that holds no
// relationship anywhere is still a grant.
#include <map>

#include "engine_internal.hpp"
#include "validate.hpp"

namespace aclint {

namespace {

constexpr uint32_t kReachCapFirst = 1u << 14;     // log entries (8 B) per block of the first attempt
constexpr uint32_t kReachCapMax = 1u << 24;       // ... and at most: beyond, ACL_ERR_RESOURCE_EXHAUSTED
constexpr uint32_t kReachRegionFirst = 1u << 15;  // records (8 B) of the call-wide output region of the first attempt
constexpr uint32_t kReachRegionMax = 1u << 27;    // ... and at most (1 GiB)
constexpr uint32_t kReachEager = 1u << 12;        // records copied back with the control words, before their number is known (32 KiB)

// the relations of `type` that a state of `member` stands for, with their dispatch offset from the state: the member itself, and what its expression's
// REFERENCES lead to on the same object, each one dispatch deeper (least offsets: breadth first; a reference cycle ends at its first repeat).  Arrows and
// usersets are not followed: their targets are states of their own, which the device returns.
void same_object_relations(const Schema &sc, int type, int member, std::vector<std::pair<int, uint32_t>> *out) {
    const Definition &def = sc.defs[type];
    std::vector<uint8_t> seen(def.members.size(), 0);
    std::vector<int> level{member}, next;
    seen[member] = 1;
    for (uint32_t d = 0; !level.empty() && d < kMaxLevels; d++) {
        next.clear();
        for (int m : level) {
            const Member &mem = def.members[m];
            if (!mem.is_permission) {
                out->push_back({m, d});
                continue;
            }
            std::vector<const Node *> todo{&mem.expr};
            while (!todo.empty()) {
                const Node *n = todo.back();
                todo.pop_back();
                if (n->kind == Node::kUnion) {
                    for (const Node &k : n->kids) todo.push_back(&k);
                } else if (n->kind == Node::kRef) {
                    const int tm = def.find(n->a);
                    if (tm >= 0 && !seen[tm]) {
                        seen[tm] = 1;
                        next.push_back(tm);
                    }
                }
            }
        }
        level.swap(next);
    }
}

// stable counting sort by level (1..kMaxLevels): in -> *out (same size)
void by_level(const std::vector<acl_grant_t> &in, std::vector<acl_grant_t> *out) {
    uint32_t at[kMaxLevels + 2] = {};
    for (const acl_grant_t &g : in) at[std::min<uint32_t>(g.level, kMaxLevels) + 1]++;
    for (uint32_t l = 1; l < kMaxLevels + 2; l++) at[l] += at[l - 1];
    for (const acl_grant_t &g : in) (*out)[at[std::min<uint32_t>(g.level, kMaxLevels)]++] = g;
}

// stable sort by (rtype, relation, rid): least-significant-digit radix over the 64-bit key, a byte at a time, bytes that all keys share skipped;
// *a is sorted through the scratch *b (same size); the result is in *a
void by_relationship(std::vector<acl_grant_t> *a, std::vector<acl_grant_t> *b) {
    auto key = [](const acl_grant_t &g) { return ((uint64_t)g.rtype << 48) | ((uint64_t)g.relation << 32) | g.rid; };
    const size_t n = a->size();
    if (n < 64) {
        std::stable_sort(a->begin(), a->end(), [&](const acl_grant_t &x, const acl_grant_t &y) { return key(x) < key(y); });
        return;
    }
    for (int byte = 0; byte < 8; byte++) {
        size_t at[257] = {};
        for (const acl_grant_t &g : *a) at[((key(g) >> (8 * byte)) & 0xFFu) + 1]++;
        bool one = false;
        for (int d = 1; d < 257; d++) one = one || at[d] == n;
        if (one) continue;
        for (int d = 1; d < 257; d++) at[d] += at[d - 1];
        for (const acl_grant_t &g : *a) (*b)[at[(key(g) >> (8 * byte)) & 0xFFu]++] = g;
        a->swap(*b);
    }
}

}  // namespace

void denial_grants(const Schema &sc, const uint2 *recs, size_t n, int stype, int srel, std::vector<acl_grant_t> *out) {
    out->clear();
    // per slot, once: the relations of the same object that accept the subject's class by name (a `T:*` class does not), with their offsets
    std::vector<std::vector<std::pair<int, uint32_t>>> rels(sc.nslots);
    std::vector<uint8_t> known(sc.nslots, 0);
    for (size_t i = 0; i < n; i++) {
        const uint32_t slot = recs[i].y & 0xFFFFu, level = (recs[i].y >> 16) & 63u;
        if (slot >= (uint32_t)sc.nslots || level == 0) continue;
        const int type = sc.slot_owner[slot].first;
        if (!known[slot]) {
            known[slot] = 1;
            std::vector<std::pair<int, uint32_t>> all;
            same_object_relations(sc, type, sc.slot_owner[slot].second, &all);
            for (const auto &r : all)
                for (const SubjectClass &c : sc.defs[type].members[r.first].classes)
                    if (!c.wildcard && c.stype == stype && c.srel == srel) {
                        rels[slot].push_back(r);
                        break;
                    }
        }
        for (const auto &r : rels[slot])
            if (level + r.second <= kMaxLevels) out->push_back(acl_grant_t{(uint16_t)type, (uint16_t)r.first, recs[i].x, level + r.second});
    }
    // Three stable passes instead of two comparison sorts (a closure of 1 000 groups is a list of 1 000 grants, and a call holds one list per resource and
    // subject class): by level; by (rtype, relation, rid) -- equals now stand in ascending levels, the first of them is kept; by level again.
    std::vector<acl_grant_t> tmp(out->size());
    by_level(*out, &tmp);
    by_relationship(&tmp, out);
    tmp.erase(std::unique(tmp.begin(), tmp.end(), [](const acl_grant_t &a, const acl_grant_t &b) { return a.rtype == b.rtype && a.relation == b.relation && a.rid == b.rid; }),
              tmp.end());
    out->resize(tmp.size());
    by_level(tmp, out);
}

namespace {

// walks the closures of roots[] = {resource id, target slot}, one block each, and hands every root's states to on_root(index, records, count), which may
// run on several host threads at once (for different roots)
template <typename OnRoot>
int reach_walk(acl_engine *h, PassCtx *c, const std::vector<uint2> &roots, OnRoot on_root) {
    const DevSubjects g = dev_subjects(h, c);
    const BlockWalk w{"Explain denial", "resource", 2 /* (8-byte log entries) */, 0, kReachCapFirst, kReachCapMax};
    uint32_t &region = c->reach_region;  // (kept across calls: a graph whose closures outgrew the first region once does not pay the redo again)
    if (region < kReachRegionFirst) region = kReachRegionFirst;
    std::vector<uint2> spans;
    return block_walk_chunks(
        h, c, w, roots.size(),
        [&](size_t b, size_t m) {
            HIP_TRY(c->d_sids.ensure(2 * m));
            HIP_TRY(c->d_subj_flags.ensure(4 + 2 * m));  // total (64 bits) | overflow | pad | the blocks' spans
            HIP_TRY(c->d_reach_recs.ensure(region));
            HIP_TRY(c->h_in.ensure(m * sizeof(uint2)));
            HIP_TRY(c->h_out.ensure(16 + m * sizeof(uint2) + kReachEager * sizeof(uint2)));
            std::memcpy(c->h_in.p, roots.data() + b, m * sizeof(uint2));
            HIP_TRY(hipMemcpyAsync(c->d_sids.p, c->h_in.p, m * sizeof(uint2), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemsetAsync(c->d_subj_flags.p, 0, 16 + m * sizeof(uint2), c->stream));  // (a block that never ran leaves an empty span)
            return (int)ACL_OK;
        },
        [&](size_t m, uint32_t cap) {
            const DevReachOut out{c->d_reach_recs.p, region, (unsigned long long *)c->d_subj_flags.p, (uint2 *)(c->d_subj_flags.p + 4), c->d_subj_flags.p + 2};
            ev_begin(c, 0);
            launch_reach_local(c->stream, g, (const uint2 *)c->d_sids.p, (uint32_t)m, c->d_fbuf[0].p, cap, c->d_subj_visited.p, out, c->d_status.p);
            ev_end(c);
            HIP_TRY(hipGetLastError());
            // control words and spans in one copy; the first records ride along, so that a small answer needs no second round trip
            HIP_TRY(hipMemcpyAsync(c->h_out.p, c->d_subj_flags.p, 16 + m * sizeof(uint2), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync((char *)c->h_out.p + 16 + m * sizeof(uint2), c->d_reach_recs.p, std::min<size_t>(region, kReachEager) * sizeof(uint2), hipMemcpyDeviceToHost,
                                   c->stream));
            return (int)ACL_OK;
        },
        [&](size_t b, size_t m) {
            const uint64_t total = *(const uint64_t *)c->h_out.p;
            const uint32_t overflow = ((const uint32_t *)c->h_out.p)[2];
            if (overflow || total > region) {  // a block's states did not fit: the same chunk again, with a larger region
                c->stats.overflow_retries++;
                if (region >= kReachRegionMax)
                    return fail(ACL_ERR_RESOURCE_EXHAUSTED, "Explain denial: the states of one pass outgrew their region (2^27 records): ask about fewer resources per call");
                region = std::min<uint64_t>((uint64_t)region * 8u, kReachRegionMax);
                return kRedoChunk;
            }
            const uint2 *recs = (const uint2 *)((const char *)c->h_out.p + 16 + m * sizeof(uint2));
            spans.assign((const uint2 *)((const char *)c->h_out.p + 16), (const uint2 *)((const char *)c->h_out.p + 16) + m);
            if (total > kReachEager) {  // (h_out is reused: the spans were copied out of it first)
                HIP_TRY(c->h_out.ensure(total * sizeof(uint2)));
                HIP_TRY(hipMemcpyAsync(c->h_out.p, c->d_reach_recs.p, total * sizeof(uint2), hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                recs = (const uint2 *)c->h_out.p;
            }
            for (size_t i = 0; i < m; i++)
                if ((uint64_t)spans[i].x + spans[i].y > total || spans[i].y == 0)  // (every walk returns at least its root)
                    return fail(ACL_ERR_INTERNAL, "Explain denial: the walk of resource id " + std::to_string(roots[b + i].x) + " returned no states of its own");
            // (the roots' lists are independent of each other: spread over the host's threads, as a list response's bytes are)
            host_parallel(h, m, 16, [&](size_t i0, size_t i1) {
                for (size_t i = i0; i < i1; i++) on_root(b + i, recs + spans[i].x, (size_t)spans[i].y);
            });
            return check_opts(c->opts);
        });
}

// caller holds an Eval with the subject rows current
int denial_batch(acl_engine *h, PassCtx *c, const acl_item_t *items, size_t n, uint8_t *perm, int32_t *err, uint8_t *flags, uint32_t *grant_off, acl_grant_t **grants_out) {
    const Schema &sc = h->store.schema();
    int rc = check_ids_chunked(h, c, items, n, perm, err);
    if (rc) return rc;
    // ---- the denied items of monotone slots, grouped: one walk per (resource type, resource id, permission), one grant list per (walk, subject class)
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> root_of;             // {slot, resource id} -> root
    std::vector<uint2> roots;
    std::vector<std::map<uint32_t, uint32_t>> lists_of;                     // [root]: subject key -> grant list
    std::vector<std::pair<int, int>> list_class;                            // [list] (stype, srel)
    std::vector<std::vector<uint32_t>> root_lists;                          // [root] its lists
    std::vector<uint32_t> item_list(n, 0xFFFFFFFFu);
    rc = explain_classify(h, "Explain denial", ACL_PERM_NO_PERMISSION, items, n, perm, err, flags, [&](size_t i, const acl_item_t &it, uint32_t slot, bool nonmono) {
        flags[i] = nonmono ? ACL_EXPLAIN_UNSUPPORTED : ACL_EXPLAIN_DENIAL;
        if (nonmono) return;
        auto r = root_of.emplace(std::make_pair(slot, it.resource_id), (uint32_t)roots.size());
        if (r.second) {
            roots.push_back(make_uint2(it.resource_id, slot));
            lists_of.emplace_back();
            root_lists.emplace_back();
        }
        const uint32_t root = r.first->second;
        const int srel = it.subject_relation == ACL_NO_RELATION ? kNoRelation : (int)it.subject_relation;
        auto l = lists_of[root].emplace(sc.subject_key(it.subject_type, srel), (uint32_t)list_class.size());
        if (l.second) {
            list_class.push_back({(int)it.subject_type, srel});
            root_lists[root].push_back(l.first->second);
        }
        item_list[i] = l.first->second;
    });
    if (rc) return rc;
    std::vector<std::vector<acl_grant_t>> lists(list_class.size());
    rc = reach_walk(h, c, roots, [&](size_t root, const uint2 *recs, size_t cnt) {
        for (uint32_t l : root_lists[root]) denial_grants(sc, recs, cnt, list_class[l].first, list_class[l].second, &lists[l]);
    });
    if (rc) return rc;
    uint64_t total = 0;
    grant_off[0] = 0;
    for (size_t i = 0; i < n; i++) {
        if (item_list[i] != 0xFFFFFFFFu) total += lists[item_list[i]].size();
        if (total > 0xFFFFFFFFull) return fail(ACL_ERR_RESOURCE_EXHAUSTED, "Explain denial: more than 2^32 grants in one call: ask about fewer items");
        grant_off[i + 1] = (uint32_t)total;
    }
    acl_grant_t *out = nullptr;
    rc = result_block(total, "out of host memory for the grants", &out);
    if (rc) return rc;
    // (every item gets its own copy of its list -- 4 096 items about one resource are 4 096 copies: the pages are touched and filled by several threads)
    host_parallel(h, n, 64, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) {
            if (item_list[i] == 0xFFFFFFFFu) continue;
            const std::vector<acl_grant_t> &l = lists[item_list[i]];
            if (!l.empty()) std::memcpy(out + grant_off[i], l.data(), l.size() * sizeof(acl_grant_t));
        }
    });
    *grants_out = out;
    return ACL_OK;
}

}  // namespace

}  // namespace aclint

int acl_explain_denial_bulk_ids(acl_engine_t *h, const acl_item_t *items, size_t n, uint8_t *perm_out, int32_t *err_out, uint8_t *flags_out, uint32_t *grant_off_out,
                                acl_grant_t **grants_out, const acl_call_opts_t *opts) {
    return explain_front(
        h, "acl_explain_denial_bulk_ids", items, n, perm_out, err_out, flags_out, opts,
        [&](PassCtx *c, int32_t *err, uint8_t *flags) { return denial_batch(h, c, items, n, perm_out, err, flags, grant_off_out, grants_out); },
        ExplainOut<acl_grant_t>{grant_off_out, grants_out});
}

// The subject of a grant is spelled as the item spelled it, and so is the item's own resource (neither needs a name in the tables: an unknown object is a
// valid one to write about); every other object of a grant takes part in relationships, so its name stays -- read under the names lock, as a witness's.
static int denial_grants_text(acl_engine_t *h, const acl_check_item_t &item, const acl_item_t &it, const acl_grant_t *grants, uint32_t k0, uint32_t k1, std::string *text) {
    std::shared_lock<std::shared_mutex> nlk(h->names_mu);
    const Schema &sc = h->store.schema();
    for (uint32_t k = k0; k < k1; k++) {
        const acl_grant_t &g = grants[k];
        if (g.rtype >= sc.defs.size() || it.subject_type >= sc.defs.size() || g.relation >= sc.defs[g.rtype].members.size() ||
            (it.subject_relation != ACL_NO_RELATION && it.subject_relation >= sc.defs[it.subject_type].members.size()))
            return fail(ACL_ERR_UNAVAILABLE, "acl_explain_denial: the schema changed while the grants were named");
        const bool own = g.rtype == it.resource_type && g.rid == it.resource_id;
        const std::string *rn = own ? nullptr : h->store.objects(g.rtype).name(g.rid);
        if (!own && !rn)
            return fail(ACL_ERR_UNAVAILABLE, "acl_explain_denial: an object of the grants has no name (loaded by id, or renamed by a write since the walk): use acl_explain_denial_bulk_ids, or ask again");
        relationship_line(sc, g.rtype, own ? std::string(item.resource_id) : *rn, g.relation, it.subject_type, item.subject_id, it.subject_relation, text);
    }
    return ACL_OK;
}

int acl_explain_denial(acl_engine_t *h, const acl_check_item_t *item, uint8_t *perm_out, int32_t *err_out, uint32_t *flags_out, char **text_out,
                       const acl_call_opts_t *opts) {
    return explain_one_front(h, "acl_explain_denial", "out of host memory for the grants", item, perm_out, err_out, flags_out, text_out,
                             [&](const acl_item_t &it, uint8_t *flag, std::string *text) {
                                 uint8_t fl = 0;
                                 uint32_t off[2] = {0, 0};
                                 acl_grant_t *grants = nullptr;
                                 int rc = acl_explain_denial_bulk_ids(h, &it, 1, perm_out, err_out, &fl, off, &grants, opts);
                                 if (rc) return rc;
                                 *flag = fl;
                                 rc = denial_grants_text(h, *item, it, grants, off[0], off[1], text);
                                 std::free(grants);
                                 return rc;
                             });
}

// Test hook: the host half alone (denial_grants) on a caller-supplied list of states.  Reads nothing but the schema: any engine will do.
int acl_selfcheck_denial_grants(acl_engine_t *h, int rtype, int member, int stype, int srel, const uint32_t *states, size_t n, acl_grant_t **grants_out, size_t *n_out) {
    if (!h || !grants_out || !n_out || (n && !states)) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_selfcheck_denial_grants: bad argument");
    *grants_out = nullptr;
    *n_out = 0;
    std::shared_lock<RwLock> slk(h->state_mu);
    if (!h->store.has_schema()) return fail(ACL_ERR_FAILED_PRECONDITION, "no schema loaded");
    const Schema &sc = h->store.schema();
    if (rtype < 0 || rtype >= (int)sc.defs.size() || stype < 0 || stype >= (int)sc.defs.size() || member < 0 || member >= (int)sc.defs[rtype].members.size() || srel < -1 ||
        srel >= (int)sc.defs[stype].members.size())
        return fail(ACL_ERR_FAILED_PRECONDITION, "acl_selfcheck_denial_grants: unknown type, member or subject relation");
    std::vector<uint2> recs(n);
    for (size_t i = 0; i < n; i++) {
        recs[i] = make_uint2(states[2 * i], states[2 * i + 1]);
        if ((recs[i].y & 0xFFFFu) >= (uint32_t)sc.nslots || ((recs[i].y >> 16) & 63u) == 0 || ((recs[i].y >> 16) & 63u) > kMaxLevels || (recs[i].y >> 22))
            return fail(ACL_ERR_INVALID_ARGUMENT, "acl_selfcheck_denial_grants: state " + std::to_string(i) + " names no slot, or a level outside 1..50");
    }
    std::vector<acl_grant_t> grants;
    denial_grants(sc, recs.data(), n, stype, srel < 0 ? kNoRelation : srel, &grants);
    const int rc = result_copy(grants.data(), grants.size(), "out of host memory for the grants", grants_out);
    if (!rc) *n_out = grants.size();
    return rc;
}

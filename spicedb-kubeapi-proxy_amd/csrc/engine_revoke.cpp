// engine_revoke.cpp -- Explain for revocation (include/aclgpu.h acl_explain_revoke*): Check + every single stored relationship whose delete revokes a granted item.
//
// A relationship whose delete, alone, turns a HAS on a monotone permission into something else lies on EVERY chain that grants the item -- so it lies on the
// one witness Explain returns.  The candidates of an item are therefore the at most 50 hops of its witness, and hop r is a cut iff the walk that leaves r out
// no longer finds the subject within the 50 dispatch levels.  One Eval holds the call: the batch is answered by the ordinary Check (check_ids_host), the
// granted monotone items get their witness from explain_walk, and k_revoke_local (kernels.hip) walks every (item, distinct hop) once more, one block each,
// with that hop masked wherever a row holds it -- all of a chunk's walks in one launch.  Nothing is written and the snapshot does not change.
//
// The mask is by RELATIONSHIP, not by op: the device compares the class of relationships an op reads (one number per op, classes_of below: resource type,
// relation, subject type, subject relation, and whether the class is a `T:*` class) and the two ends.  `view = viewer + edit`, `edit = viewer` reads one
// viewer relationship through several ops; every one of them skips it.
#include <map>
#include <tuple>

#include "engine_internal.hpp"
#include "validate.hpp"

namespace aclint {

namespace {

constexpr uint32_t kRevokeCapFirst = 1u << 14;  // log entries (8 B) per block of the first attempt
constexpr uint32_t kRevokeCapMax = 1u << 24;    // ... and at most: beyond, ACL_ERR_RESOURCE_EXHAUSTED
constexpr uint32_t kNoClass = 0xFFFFFFFFu;      // an op that reads no relationships (no mask carries it)

using ClassKey = std::tuple<uint16_t, uint16_t, uint16_t, uint16_t, bool>;  // (rtype, relation, stype, srel, `T:*`)

// numbers the classes of relationships the programs' ops read: *of_op per op (kNoClass: none), *of_key for the hops
void classes_of(const acl_engine *h, std::vector<uint32_t> *of_op, std::map<ClassKey, uint32_t> *of_key) {
    const std::vector<ExplainOp> &x = h->subj.xops;
    of_op->assign(x.size(), kNoClass);
    for (size_t j = 0; j < x.size(); j++) {
        if (x[j].rtype == ExplainOp::kExplainRewrite) continue;
        const ClassKey key{x[j].rtype, x[j].relation, x[j].stype, x[j].srel, (h->snap.ops[j].flags & OP_WILD) != 0u};
        (*of_op)[j] = of_key->emplace(key, (uint32_t)of_key->size()).first->second;
    }
}

bool same_relationship(const acl_explain_hop_t &a, const acl_explain_hop_t &b) {
    return a.rtype == b.rtype && a.relation == b.relation && a.rid == b.rid && a.stype == b.stype && a.srel == b.srel && a.sid == b.sid &&
           (a.flags & ACL_HOP_WILDCARD) == (b.flags & ACL_HOP_WILDCARD);
}

struct MaskedWalk {  // one block of k_revoke_local
    uint32_t pick;   // index into `pick` (the item)
    uint32_t hop;    // index into the call's distinct hops
    uint32_t cls;
};

// caller holds an Eval with the subject rows current
int revoke_batch(acl_engine *h, PassCtx *c, const acl_item_t *items, size_t n, uint8_t *perm, int32_t *err, uint8_t *flags, uint32_t *cut_off, acl_explain_hop_t **cuts_out) {
    const Schema &sc = h->store.schema();
    int rc = check_ids_chunked(h, c, items, n, perm, err);
    if (rc) return rc;
    std::vector<uint32_t> pick;
    rc = explain_classify(h, "Explain revoke", ACL_PERM_HAS_PERMISSION, items, n, perm, err, flags, [&](size_t i, const acl_item_t &, uint32_t, bool nonmono) {
        if (nonmono) flags[i] = ACL_EXPLAIN_UNSUPPORTED;
        else pick.push_back((uint32_t)i);
    });
    if (rc) return rc;
    // ---- the witnesses: the candidates
    std::vector<acl_explain_hop_t> hops;
    std::vector<uint32_t> count;
    rc = explain_walk(h, c, items, pick, &hops, &count);
    if (rc) return rc;
    // ---- one masked walk per (item, distinct hop), in witness order
    std::vector<uint32_t> of_op;
    std::map<ClassKey, uint32_t> of_key;
    classes_of(h, &of_op, &of_key);
    std::vector<acl_explain_hop_t> cand;  // the distinct hops of all items, item after item
    std::vector<MaskedWalk> walks;
    size_t at = 0;
    for (size_t k = 0; k < pick.size(); k++) {
        const size_t first = cand.size();
        for (uint32_t j = 0; j < count[k]; j++) {
            const acl_explain_hop_t &hp = hops[at + j];
            bool seen = false;
            for (size_t q = first; q < cand.size() && !seen; q++) seen = same_relationship(cand[q], hp);
            if (seen) continue;  // (a relationship that occurs twice in a witness is one candidate)
            const auto cl = of_key.find(ClassKey{hp.rtype, hp.relation, hp.stype, hp.srel, (hp.flags & ACL_HOP_WILDCARD) != 0u});
            if (cl == of_key.end())
                return fail(ACL_ERR_INTERNAL, "Explain revoke: a hop of the witness of " + explain_item_text(items[pick[k]], pick[k]) + " is of a class no op reads");
            walks.push_back(MaskedWalk{(uint32_t)k, (uint32_t)cand.size(), cl->second});
            cand.push_back(hp);
        }
        at += count[k];
    }
    if (walks.size() >= 0xFFFFFFFFull) return fail(ACL_ERR_RESOURCE_EXHAUSTED, "Explain revoke: more than 2^32 masked walks in one call: ask about fewer items");
    std::vector<uint8_t> is_cut(walks.size(), 0);
    const DevState &d = *c->dev;
    const DevSubjects g = dev_subjects(h, c);
    const size_t nops = of_op.size();
    if (nops != h->snap.ops.size()) return fail(ACL_ERR_INTERNAL, "Explain revoke: the per-op side table does not match the programs");
    const BlockWalk w{"Explain revoke", "item with one relationship left out", 2 /* (8-byte log entries) */, 0, kRevokeCapFirst, kRevokeCapMax};
    rc = block_walk_chunks(
        h, c, w, walks.size(),
        [&](size_t b, size_t m) {
            HIP_TRY(c->d_items.ensure(2 * m));
            HIP_TRY(c->d_sids.ensure(std::max<size_t>(nops, 1)));
            HIP_TRY(c->d_subj_flags.ensure(m));
            HIP_TRY(c->h_in.ensure(2 * m * sizeof(uint4) + nops * 4));
            HIP_TRY(c->h_out.ensure(m * 4));
            uint4 *recs = (uint4 *)c->h_in.p;
            for (size_t i = 0; i < m; i++) {
                const MaskedWalk &mw = walks[b + i];
                const acl_item_t &it = items[pick[mw.pick]];
                const acl_explain_hop_t &hp = cand[mw.hop];
                const uint32_t key = sc.subject_key(it.subject_type, it.subject_relation == ACL_NO_RELATION ? kNoRelation : (int)it.subject_relation);
                recs[2 * i] = make_uint4(it.resource_id, (uint32_t)sc.slot(it.resource_type, it.permission), key, it.subject_id);
                recs[2 * i + 1] = make_uint4(mw.cls, hp.rid, hp.sid, (hp.flags & ACL_HOP_WILDCARD) ? 1u : 0u);
            }
            uint32_t *cls_in = (uint32_t *)(recs + 2 * m);
            if (nops) std::memcpy(cls_in, of_op.data(), nops * 4);
            HIP_TRY(hipMemcpyAsync(c->d_items.p, recs, 2 * m * sizeof(uint4), hipMemcpyHostToDevice, c->stream));
            if (nops) HIP_TRY(hipMemcpyAsync(c->d_sids.p, cls_in, nops * 4, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemsetAsync(c->d_subj_flags.p, 0xFF, m * 4, c->stream));  // (a block that never ran answers neither way)
            return (int)ACL_OK;
        },
        [&](size_t m, uint32_t cap) {
            ev_begin(c, 0);
            launch_revoke_local(c->stream, g, d.d_buckets.p, c->d_sids.p, c->d_items.p, (uint32_t)m, c->d_fbuf[0].p, cap, c->d_subj_visited.p, c->d_subj_flags.p, c->d_status.p);
            ev_end(c);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(c->h_out.p, c->d_subj_flags.p, m * 4, hipMemcpyDeviceToHost, c->stream));
            return (int)ACL_OK;
        },
        [&](size_t b, size_t m) {
            const uint32_t *found = (const uint32_t *)c->h_out.p;
            for (size_t i = 0; i < m; i++) {
                if (found[i] == kRevokeNotFound) is_cut[b + i] = 1;
                else if (found[i] != kRevokeFound) {
                    const uint32_t idx = pick[walks[b + i].pick];
                    return fail(ACL_ERR_INTERNAL, "Explain revoke: a walk of " + explain_item_text(items[idx], idx) + " with one relationship left out neither found the subject nor ran dry");
                }
            }
            return (int)ACL_OK;
        });
    if (rc) return rc;
    std::fill(cut_off, cut_off + n + 1, 0u);
    std::vector<acl_explain_hop_t> cuts;
    for (size_t q = 0; q < walks.size(); q++) {
        if (!is_cut[q]) continue;
        cut_off[pick[walks[q].pick] + 1]++;
        cuts.push_back(cand[walks[q].hop]);  // (walks stand item after item, in witness order: so do the cuts)
    }
    for (size_t k = 0; k < pick.size(); k++) flags[pick[k]] = ACL_EXPLAIN_REVOKE;
    for (size_t i = 0; i < n; i++) cut_off[i + 1] += cut_off[i];
    return result_copy(cuts.data(), cuts.size(), "out of host memory for the cuts", cuts_out);
}

}  // namespace

}  // namespace aclint

int acl_explain_revoke_bulk_ids(acl_engine_t *h, const acl_item_t *items, size_t n, uint8_t *perm_out, int32_t *err_out, uint8_t *flags_out, uint32_t *cut_off_out,
                                acl_explain_hop_t **cuts_out, const acl_call_opts_t *opts) {
    return explain_front(
        h, "acl_explain_revoke_bulk_ids", items, n, perm_out, err_out, flags_out, opts,
        [&](PassCtx *c, int32_t *err, uint8_t *flags) { return revoke_batch(h, c, items, n, perm_out, err, flags, cut_off_out, cuts_out); },
        ExplainOut<acl_explain_hop_t>{cut_off_out, cuts_out});
}

int acl_explain_revoke(acl_engine_t *h, const acl_check_item_t *item, uint8_t *perm_out, int32_t *err_out, uint32_t *flags_out, char **text_out,
                       const acl_call_opts_t *opts) {
    return explain_one_front(h, "acl_explain_revoke", "out of host memory for the cuts", item, perm_out, err_out, flags_out, text_out,
                             [&](const acl_item_t &it, uint8_t *flag, std::string *text) {
                                 uint8_t fl = 0;
                                 uint32_t off[2] = {0, 0};
                                 acl_explain_hop_t *cuts = nullptr;
                                 int rc = acl_explain_revoke_bulk_ids(h, &it, 1, perm_out, err_out, &fl, off, &cuts, opts);
                                 if (rc) return rc;
                                 *flag = fl;
                                 rc = explain_hops_text(h, "acl_explain_revoke", cuts, off[0], off[1], text);
                                 std::free(cuts);
                                 return rc;
                             });
}

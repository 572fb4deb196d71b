// plan_subjects.cpp -- subject rows + the per-op side table of LookupSubjects (kernels.hip k_subj_local).  See plan.hpp SubjectRows.
// The walk interprets the FORWARD programs from the resource down; the only data it lacks is the list of subjects of a membership-only class,
// whose rows (plan.cpp) are indexed by subject.  Those are transposed here: the class's keys ascend by (resource, subject), so each resource's
// subjects come out ascending as they are read.
#include <algorithm>

#include "plan.hpp"

namespace acl {

std::vector<uint8_t> subject_skip_ops(const Snapshot &s) {
    std::vector<uint8_t> skip(s.ops.size(), 0);
    for (const SlotProg &p : s.progs) {
        if (!p.combine) continue;
        // the boolean program in postfix: which leaves sit (at any nesting) inside the subtracted operand of an exclusion
        const uint32_t *bx = s.bexpr.data() + p.combine;
        const uint32_t ntok = bx[0];
        const uint32_t *tok = bx + 1 + (p.nleaves + 1);
        std::vector<uint8_t> excluded(p.nleaves + 1, 0);
        std::vector<std::vector<uint32_t>> st;  // the leaves under each value on the stack
        for (uint32_t i = 0; i < ntok; i++) {
            const uint32_t t = tok[i], kind = t & 0xFF000000u, arg = t & 0xFFFFFFu;
            if (kind == BX_LEAF || kind == BX_LEAF_ALL) {
                st.push_back({arg});
            } else if (kind == BX_OR || kind == BX_AND) {
                std::vector<uint32_t> u;
                for (uint32_t k = 0; k < arg && !st.empty(); k++) {
                    u.insert(u.end(), st.back().begin(), st.back().end());
                    st.pop_back();
                }
                st.push_back(std::move(u));
            } else if (kind == BX_EXCL && st.size() >= 2) {
                std::vector<uint32_t> sub = std::move(st.back());
                st.pop_back();
                for (uint32_t l : sub)
                    if (l <= p.nleaves) excluded[l] = 1;
                st.back().insert(st.back().end(), sub.begin(), sub.end());
            }
        }
        for (uint32_t j = 0; j < p.n_total; j++) {
            const FwdOp &op = s.ops[p.first + j];
            if (op.leaf && op.leaf <= p.nleaves && excluded[op.leaf]) skip[p.first + j] = 1;
        }
    }
    return skip;
}

std::vector<ExplainOp> explain_ops(const Schema &sc, const Snapshot &s) {
    // a hashed op names its class by the descriptor base of the class's hashed rows, a sorted op by its relation's descriptor base + its sorted-class index
    struct Cls {
        uint32_t base, k;
        bool hashed;
        ExplainOp x;
    };
    std::vector<Cls> cls;
    for (int slot = 0; slot < sc.nslots && (size_t)slot < s.lay.size(); slot++) {
        const RelLayout &l = s.lay[slot];
        const Member &m = sc.defs[sc.slot_owner[slot].first].members[sc.slot_owner[slot].second];
        for (size_t k = 0; k < l.cls.size() && k < m.classes.size(); k++) {
            const ClassLayout &c = l.cls[k];
            if (!c.live) continue;
            ExplainOp x;
            x.rtype = (uint16_t)sc.slot_owner[slot].first;
            x.relation = (uint16_t)sc.slot_owner[slot].second;
            x.stype = (uint16_t)m.classes[k].stype;
            x.srel = m.classes[k].srel == kNoRelation ? (uint16_t)0xFFFFu : (uint16_t)m.classes[k].srel;
            cls.push_back(Cls{c.hashed ? c.smeta_base : l.meta_base, c.hashed ? 0u : c.ks, c.hashed, x});
        }
    }
    std::vector<ExplainOp> out(s.ops.size());
    for (size_t j = 0; j < s.ops.size(); j++) {
        const FwdOp &op = s.ops[j];
        if (!(op.flags & (OP_PROBE | OP_ENUM | OP_PROBE_HASH)) || (op.flags & (OP_PUSH_SAME | OP_REFLEX))) continue;
        const bool hashed = (op.flags & OP_PROBE_HASH) != 0;
        for (const Cls &c : cls)
            if (c.hashed == hashed && c.base == op.base && (hashed || c.k == op.k)) {
                out[j] = c.x;
                break;
            }
    }
    return out;
}

void build_subjects(Store &store, int64_t now, const Snapshot &s, SubjectRows *out) {
    const Schema &sc = store.schema();
    SubjectRows r;
    auto &tables = store.tables();
    r.smeta.assign(2, 0);  // (descriptor 0: nobody's, empty)
    r.sops.assign(s.ops.size(), SubjOp{});
    r.type_cover.assign(sc.defs.size(), 0);
    for (size_t t = 0; t < sc.defs.size(); t++) r.type_cover[t] = store.objects((int)t).count();
    // ---- per (slot, hashed class): resource -> ascending subject ids
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> cls_rows(sc.nslots);  // [slot][class] {first descriptor, resource ids covered}
    for (int slot = 0; slot < sc.nslots && (size_t)slot < s.lay.size(); slot++) {
        const RelLayout &l = s.lay[slot];
        cls_rows[slot].assign(l.cls.size(), {0u, 0u});
        for (size_t k = 0; k < l.cls.size(); k++) {
            const ClassLayout &c = l.cls[k];
            if (!c.live || !c.hashed) continue;
            const ClassTable &ct = tables[slot][k];
            const bool filt = !ct.expiry.empty();
            const uint32_t nres = std::max(l.nrows, with_headroom(store.objects(sc.slot_owner[slot].first).count()));
            const uint32_t base = (uint32_t)(r.smeta.size() / 2);
            r.smeta.resize(r.smeta.size() + 2 * (size_t)nres, 0);
            uint32_t *md = r.smeta.data() + 2 * (size_t)base;
            const size_t nk = ct.keys.size();
            size_t i = 0;
            while (i < nk) {
                const uint32_t res = (uint32_t)(ct.keys[i] >> 32);
                const uint32_t start = (uint32_t)r.sids.size();
                for (; i < nk && (uint32_t)(ct.keys[i] >> 32) == res; i++)
                    if (!filt || store.live(ct, ct.keys[i], now)) r.sids.push_back((uint32_t)ct.keys[i]);
                if (res < nres) {
                    md[2 * (size_t)res] = start;
                    md[2 * (size_t)res + 1] = (uint32_t)r.sids.size();
                } else {
                    r.sids.resize(start);
                }
            }
            cls_rows[slot][k] = {base, nres};
        }
    }
    if (r.sids.empty()) r.sids.push_back(0);
    // ---- side table: every OP_PROBE_HASH op finds its class's subject rows by the hashed rows' descriptor base (unique per class)
    std::vector<std::pair<uint32_t, uint32_t>> by_smeta;  // {ClassLayout::smeta_base, index into a flat list}
    std::vector<std::pair<uint32_t, uint32_t>> flat;
    for (int slot = 0; slot < sc.nslots && (size_t)slot < s.lay.size(); slot++)
        for (size_t k = 0; k < s.lay[slot].cls.size(); k++) {
            const ClassLayout &c = s.lay[slot].cls[k];
            if (!c.live || !c.hashed) continue;
            by_smeta.push_back({c.smeta_base, (uint32_t)flat.size()});
            flat.push_back(cls_rows[slot][k]);
        }
    std::sort(by_smeta.begin(), by_smeta.end());
    const std::vector<uint8_t> skip = subject_skip_ops(s);
    for (size_t j = 0; j < s.ops.size(); j++) {
        const FwdOp &op = s.ops[j];
        SubjOp &so = r.sops[j];
        so.flags = skip[j] ? kSubjSkip : 0u;
        if (!(op.flags & OP_PROBE_HASH)) continue;
        auto it = std::lower_bound(by_smeta.begin(), by_smeta.end(), std::make_pair(op.base, 0u));
        if (it == by_smeta.end() || it->first != op.base) continue;  // (cannot happen: every hashed op names a live class)
        so.base = flat[it->second].first;
        so.nrows = flat[it->second].second;
    }
    r.xops = explain_ops(sc, s);
    // ---- visited bits: only slots some op produces children in (the resource's own state is the walk's root and is expanded once)
    r.slot_vbase.assign(sc.nslots, kSubjNoBits);
    r.slot_vn.assign(sc.nslots, 0);
    std::vector<uint8_t> child(sc.nslots, 0);
    for (const FwdOp &op : s.ops)
        if ((op.flags & (OP_ENUM | OP_PUSH_SAME)) && op.key < (uint32_t)sc.nslots) child[op.key] = 1;
    // A shard's programs hold row ops only for the types it owns, but its states are also the children of rows on OTHER shards (pod#viewer@group#member
    // lives with `pod`, the group#member states it produces with `group`): there the producers are read off the schema -- the userset classes and the
    // arrows of every definition, which is what the owners' programs enumerate (computed usersets stay on their own object, hence on its shard).
    bool sharded = false;
    for (uint32_t o : s.type_owner) sharded = sharded || o != s.type_owner[0];
    if (sharded) {
        std::vector<std::pair<int, const Node *>> todo;
        for (size_t t = 0; t < sc.defs.size(); t++)
            for (const Member &m : sc.defs[t].members) {
                if (m.is_permission) todo.push_back({(int)t, &m.expr});
                for (const SubjectClass &c : m.classes)
                    if (c.srel != kNoRelation) child[sc.slot(c.stype, c.srel)] = 1;
            }
        while (!todo.empty()) {
            const auto [t, n] = todo.back();
            todo.pop_back();
            for (const Node &k : n->kids) todo.push_back({t, &k});
            if (n->kind != Node::kArrow && n->kind != Node::kArrowAll) continue;
            const int ts = sc.defs[t].find(n->a);
            if (ts < 0) continue;
            for (const SubjectClass &c : sc.defs[t].members[ts].classes) {
                const int tm = sc.defs[c.stype].find(n->b);
                if (tm >= 0) child[sc.slot(c.stype, tm)] = 1;
            }
        }
    }
    uint64_t words = 0;
    for (int slot = 0; slot < sc.nslots; slot++) {
        if (!child[slot]) continue;
        r.slot_vbase[slot] = (uint32_t)words;
        r.slot_vn[slot] = with_headroom(store.objects(sc.slot_owner[slot].first).count());
        words += ((uint64_t)r.slot_vn[slot] + 31) / 32;
    }
    r.visited_words = (uint32_t)std::max<uint64_t>(words, 1);
    for (const SlotProg &p : s.progs) {
        r.max_ops = std::max(r.max_ops, p.n_main);
        r.max_ops_rel = std::max(r.max_ops_rel, p.n_total);
    }
    *out = std::move(r);
}

}  // namespace acl

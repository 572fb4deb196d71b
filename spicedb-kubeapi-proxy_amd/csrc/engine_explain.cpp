// engine_explain.cpp -- Explain (include/aclgpu.h acl_explain*): Check + a witness chain of stored relationships for every item a monotone permission grants.
//
// One Eval holds the call: the batch is answered by the ordinary Check (check_ids_host), then the items that came back HAS on a monotone slot are walked once
// more by k_explain_local (kernels.hip), one block each, which remembers how it reached every state and stops at the level that finds the item's subject.  The
// kernel hands back (op index, parent id, child id) records in path order; the per-op side table (plan.hpp ExplainOp) names the relation and the subject class
// each op reads, which turns a record into a relationship.  Steps through a computed userset that was not inlined (OP_PUSH_SAME) stay on their object and
// produce no hop.  A granted item without a chain would be a disagreement between the two kernels: the call fails rather than return an empty witness.
#include "engine_internal.hpp"
#include "validate.hpp"

namespace aclint {

namespace {

constexpr uint32_t kExplainCapFirst = 1u << 14;  // log entries (16 B) per block of the first attempt
constexpr uint32_t kExplainCapMax = 1u << 24;    // ... and at most: beyond, ACL_ERR_RESOURCE_EXHAUSTED

}  // namespace

std::string explain_item_text(const acl_item_t &it, size_t i) {
    return "item " + std::to_string(i) + " (type " + std::to_string(it.resource_type) + " id " + std::to_string(it.resource_id) + " permission " +
           std::to_string(it.permission) + " @ type " + std::to_string(it.subject_type) + " id " + std::to_string(it.subject_id) + ")";
}

// walks the items listed in `pick` (indices into items; all HAS on a monotone slot) and appends their hops; count[k] = hops of pick[k]
// (engine_proof.cpp walks its monotone items through it too)
int explain_walk(acl_engine *h, PassCtx *c, const acl_item_t *items, const std::vector<uint32_t> &pick, std::vector<acl_explain_hop_t> *hops, std::vector<uint32_t> *count) {
    const Schema &sc = h->store.schema();
    const SubjectRows &sr = h->subj;
    const DevState &d = *c->dev;
    const DevSubjects g = dev_subjects(h, c);
    if (sr.xops.size() != h->snap.ops.size()) return fail(ACL_ERR_INTERNAL, "Explain: the per-op side table does not match the programs");
    count->assign(pick.size(), 0);
    const BlockWalk w{"Explain", "item", 1 /* (16-byte log entries) */, 0, kExplainCapFirst, kExplainCapMax};
    uint4 *h_tr = nullptr;
    uint32_t *h_cnt = nullptr;
    return block_walk_chunks(
        h, c, w, pick.size(),
        [&](size_t b, size_t m) {
            const size_t trace_words = m * kExplainTraceRecs * 4;
            HIP_TRY(c->d_items.ensure(m));
            HIP_TRY(c->d_subj_rows.ensure(trace_words));
            HIP_TRY(c->d_subj_flags.ensure(m));
            HIP_TRY(c->h_in.ensure(m * sizeof(uint4)));
            HIP_TRY(c->h_out.ensure(trace_words * 4 + m * 4));
            uint4 *recs_in = (uint4 *)c->h_in.p;
            for (size_t i = 0; i < m; i++) {
                const acl_item_t &it = items[pick[b + i]];
                const uint32_t key = sc.subject_key(it.subject_type, it.subject_relation == ACL_NO_RELATION ? kNoRelation : (int)it.subject_relation);
                recs_in[i] = make_uint4(it.resource_id, (uint32_t)sc.slot(it.resource_type, it.permission), key, it.subject_id);
            }
            HIP_TRY(hipMemcpyAsync(c->d_items.p, recs_in, m * sizeof(uint4), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemsetAsync(c->d_subj_flags.p, 0xFF, m * 4, c->stream));  // (a block that never ran leaves no "found")
            return (int)ACL_OK;
        },
        [&](size_t m, uint32_t cap) {
            const size_t trace_words = m * kExplainTraceRecs * 4;
            ev_begin(c, 0);
            launch_explain_local(c->stream, g, d.d_buckets.p, c->d_items.p, (uint32_t)m, c->d_fbuf[0].p, cap, c->d_subj_visited.p, (uint4 *)c->d_subj_rows.p,
                                 c->d_subj_flags.p, c->d_status.p);
            ev_end(c);
            HIP_TRY(hipGetLastError());
            h_tr = (uint4 *)c->h_out.p;
            h_cnt = (uint32_t *)(h_tr + m * kExplainTraceRecs);
            HIP_TRY(hipMemcpyAsync(h_tr, c->d_subj_rows.p, trace_words * 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(h_cnt, c->d_subj_flags.p, m * 4, hipMemcpyDeviceToHost, c->stream));
            return (int)ACL_OK;
        },
        [&](size_t b, size_t m) {
            for (size_t i = 0; i < m; i++) {
                const size_t idx = pick[b + i];
                const uint32_t state = h_cnt[i] >> 16, nrec = h_cnt[i] & 0xFFFFu;
                if (state != kExplainFound || nrec > kExplainTraceRecs)
                    return fail(ACL_ERR_INTERNAL, "Explain: Check grants " + explain_item_text(items[idx], idx) + " but the walk " +
                                                      (state == kExplainNotFound ? "found no chain of relationships" : "could not trace its chain back") + " (the two kernels disagree)");
                uint32_t nh = 0;
                for (uint32_t k = 0; k < nrec; k++) {
                    const uint4 r = h_tr[i * kExplainTraceRecs + k];
                    if (r.x >= sr.xops.size()) return fail(ACL_ERR_INTERNAL, "Explain: a trace record of " + explain_item_text(items[idx], idx) + " names no op");
                    const ExplainOp &x = sr.xops[r.x];
                    if (x.rtype == ExplainOp::kExplainRewrite) {
                        if (h->snap.ops[r.x].flags & OP_PUSH_SAME) continue;  // a rewrite step: same object, no relationship
                        return fail(ACL_ERR_INTERNAL, "Explain: a trace record of " + explain_item_text(items[idx], idx) + " names an op that reads no relationships");
                    }
                    hops->push_back(acl_explain_hop_t{x.rtype, x.relation, r.y, x.stype, x.srel, r.z, (r.w & kExplainRecWild) ? ACL_HOP_WILDCARD : 0u});
                    nh++;
                }
                (*count)[b + i] = nh;
            }
            return (int)ACL_OK;
        });
}

// ---- the call front the three forms share (engine_internal.hpp)
static int explain_unavailable() { return fail(ACL_ERR_UNAVAILABLE, "engine was opened store-only (no GPU): Explain is unavailable"); }

int check_ids_chunked(acl_engine *h, PassCtx *c, const acl_item_t *items, size_t n, uint8_t *perm, int32_t *err) {
    const size_t chunk = std::max<size_t>(h->max_sub_batch, 1);
    for (size_t b = 0; b < n; b += chunk) {
        int rc = check_ids_host(h, c, items + b, std::min(chunk, n - b), perm + b, err + b);
        if (rc) return rc;
    }
    return ACL_OK;
}

int explain_classify(acl_engine *h, const char *form, uint8_t want, const acl_item_t *items, size_t n, const uint8_t *perm, const int32_t *err, uint8_t *flags,
                     const std::function<void(size_t, const acl_item_t &, uint32_t, bool)> &on_item) {
    const Schema &sc = h->store.schema();
    for (size_t i = 0; i < n; i++) {
        flags[i] = 0;
        const acl_item_t &it = items[i];
        if (err[i] || perm[i] != want) continue;
        // (an item answered without error passed the device's validation; the host reads the same fields, so it checks them again before it indexes with them)
        if (it.resource_type >= sc.defs.size() || it.subject_type >= sc.defs.size() || it.permission >= sc.defs[it.resource_type].members.size() ||
            (it.subject_relation != ACL_NO_RELATION && it.subject_relation >= sc.defs[it.subject_type].members.size()))
            return fail(ACL_ERR_INTERNAL, std::string(form) + (want == ACL_PERM_HAS_PERMISSION ? ": Check grants" : ": Check answers") + " the ill-formed " + explain_item_text(it, i));
        const uint32_t slot = (uint32_t)sc.slot(it.resource_type, it.permission);
        on_item(i, it, slot, slot < h->snap.slot_nonmono.size() && h->snap.slot_nonmono[slot]);
    }
    return ACL_OK;
}

int explain_front_run(acl_engine_t *h, const std::string &fn, size_t n, int32_t *err_out, uint8_t *flags_out, const acl_call_opts_t *o, const ExplainBatch &batch) {
    if (n >= 0xFFFFFFFFull) return fail(ACL_ERR_INVALID_ARGUMENT, fn + ": too many items");
    const CallOpts opts = call_opts(o);
    if (h->store_only) return explain_unavailable();
    {
        std::shared_lock<RwLock> slk(h->state_mu);
        if (!h->store.has_schema()) return fail(ACL_ERR_FAILED_PRECONDITION, "no schema loaded");
        int rc = not_sharded(h);
        if (rc) return rc;
    }
    if (!n) return ACL_OK;
    std::vector<int32_t> err_local;
    std::vector<uint8_t> flags_local;
    if (!err_out) {
        err_local.assign(n, 0);
        err_out = err_local.data();
    }
    if (!flags_out) {
        flags_local.assign(n, 0);
        flags_out = flags_local.data();
    }
    Eval ev;
    int rc = ev.begin(h, false, opts, -1, -1, true);
    if (rc) return rc;
    rc = not_sharded(h);  // (again, now that the evaluation holds the lock: the first test let go of it)
    if (rc) return rc;
    return batch(ev.c, err_out, flags_out);
}

int explain_one_front(acl_engine_t *h, const char *fn, const char *out_of_memory, const acl_check_item_t *item, uint8_t *perm_out, int32_t *err_out, uint32_t *flags_out,
                      char **text_out, const std::function<int(const acl_item_t &, uint8_t *, std::string *)> &answer) {
    if (!item || !perm_out || !err_out || !text_out) return fail(ACL_ERR_INVALID_ARGUMENT, std::string(fn) + ": NULL argument");
    *perm_out = ACL_PERM_UNSPECIFIED;
    *err_out = 0;
    *text_out = nullptr;
    if (flags_out) *flags_out = 0;
    acl_item_t it{};
    int32_t code;
    {
        std::shared_lock<RwLock> slk(h->state_mu);
        std::shared_lock<std::shared_mutex> nlk(h->names_mu);
        if (!h->store.has_schema()) return fail(ACL_ERR_FAILED_PRECONDITION, "no schema loaded");
        code = intern_check_item(h, *item, &it);
    }
    // as acl_check_bulk: a request the API's validation refuses fails as a whole, an unknown type / permission / relation is the item's own error
    if (code == ACL_ERR_INVALID_ARGUMENT && !h->per_item_validation) return fail(ACL_ERR_INVALID_ARGUMENT, "invalid CheckPermissionRequest: a field is empty or does not match the API's pattern");
    if (h->store_only) return explain_unavailable();
    std::string text;
    if (code) {
        *err_out = code;
    } else {
        uint8_t fl = 0;
        const int rc = answer(it, &fl, &text);
        if (flags_out) *flags_out = fl;
        if (rc) return rc;
    }
    return result_copy(text.c_str(), text.size() + 1, out_of_memory, text_out);
}

namespace {

// caller holds an Eval with the subject rows current
int explain_batch(acl_engine *h, PassCtx *c, const acl_item_t *items, size_t n, uint8_t *perm, int32_t *err, uint8_t *flags, uint32_t *hop_off,
                  acl_explain_hop_t **hops_out) {
    int rc = check_ids_chunked(h, c, items, n, perm, err);
    if (rc) return rc;
    std::vector<uint32_t> pick;
    rc = explain_classify(h, "Explain", ACL_PERM_HAS_PERMISSION, items, n, perm, err, flags, [&](size_t i, const acl_item_t &, uint32_t, bool nonmono) {
        if (nonmono) flags[i] = ACL_EXPLAIN_UNSUPPORTED;
        else pick.push_back((uint32_t)i);
    });
    if (rc) return rc;
    std::vector<acl_explain_hop_t> hops;
    std::vector<uint32_t> count;
    rc = explain_walk(h, c, items, pick, &hops, &count);
    if (rc) return rc;
    std::fill(hop_off, hop_off + n + 1, 0u);
    for (size_t k = 0; k < pick.size(); k++) {
        flags[pick[k]] = ACL_EXPLAIN_WITNESS;
        hop_off[pick[k] + 1] = count[k];
    }
    for (size_t i = 0; i < n; i++) hop_off[i + 1] += hop_off[i];
    return result_copy(hops.data(), hops.size(), "out of host memory for the witness", hops_out);
}

}  // namespace

void relationship_line(const Schema &sc, uint16_t rtype, const std::string &rid, uint16_t relation, uint16_t stype, const std::string &sid, uint16_t srel, std::string *text) {
    *text += sc.defs[rtype].name + ":" + rid + "#" + sc.defs[rtype].members[relation].name + "@" + sc.defs[stype].name + ":" + sid;
    if (srel != ACL_NO_RELATION) *text += "#" + sc.defs[stype].members[srel].name;
    *text += "\n";
}

// hops [k0, k1) in the tuple grammar of aclgpu/text.py, one per line, appended to *text.  Names are read under the names lock, as acl_object_name_copy
// reads them (the hops' objects take part in relationships: their names stay)
int explain_hops_text(acl_engine *h, const char *fn, const acl_explain_hop_t *hops, uint32_t k0, uint32_t k1, std::string *text) {
    const std::string who = fn;
    std::shared_lock<std::shared_mutex> nlk(h->names_mu);
    const Schema &sc = h->store.schema();
    for (uint32_t k = k0; k < k1; k++) {
        const acl_explain_hop_t &hp = hops[k];
        if (hp.rtype >= sc.defs.size() || hp.stype >= sc.defs.size() || hp.relation >= sc.defs[hp.rtype].members.size() ||
            (hp.srel != ACL_NO_RELATION && hp.srel >= sc.defs[hp.stype].members.size()))
            return fail(ACL_ERR_UNAVAILABLE, who + ": the schema changed while the witness was named");
        const std::string *rn = h->store.objects(hp.rtype).name(hp.rid), *sn = h->store.objects(hp.stype).name(hp.sid);
        if (!rn || (!sn && !(hp.flags & ACL_HOP_WILDCARD)))  // (the evaluation has ended: a write since may have taken a hop's object away; objects loaded by id never had a name)
            return fail(ACL_ERR_UNAVAILABLE, who + ": an object of the witness has no name (loaded by id, or renamed by a write since the walk): use " + who + "_bulk_ids, or ask again");
        relationship_line(sc, hp.rtype, *rn, hp.relation, hp.stype, (hp.flags & ACL_HOP_WILDCARD) ? std::string("*") : *sn, hp.srel, text);
    }
    return ACL_OK;
}

}  // namespace aclint

int acl_explain_bulk_ids(acl_engine_t *h, const acl_item_t *items, size_t n, uint8_t *perm_out, int32_t *err_out, uint8_t *flags_out, uint32_t *hop_off_out,
                         acl_explain_hop_t **hops_out, const acl_call_opts_t *opts) {
    return explain_front(
        h, "acl_explain_bulk_ids", items, n, perm_out, err_out, flags_out, opts,
        [&](PassCtx *c, int32_t *err, uint8_t *flags) { return explain_batch(h, c, items, n, perm_out, err, flags, hop_off_out, hops_out); },
        ExplainOut<acl_explain_hop_t>{hop_off_out, hops_out});
}

int acl_explain(acl_engine_t *h, const acl_check_item_t *item, uint8_t *perm_out, int32_t *err_out, uint32_t *flags_out, char **text_out, const acl_call_opts_t *opts) {
    return explain_one_front(h, "acl_explain", "out of host memory for the witness", item, perm_out, err_out, flags_out, text_out,
                             [&](const acl_item_t &it, uint8_t *flag, std::string *text) {
                                 uint8_t fl = 0;
                                 uint32_t off[2] = {0, 0};
                                 acl_explain_hop_t *hops = nullptr;
                                 int rc = acl_explain_bulk_ids(h, &it, 1, perm_out, err_out, &fl, off, &hops, opts);
                                 if (rc) return rc;
                                 *flag = fl;
                                 rc = explain_hops_text(h, "acl_explain", hops, off[0], off[1], text);
                                 std::free(hops);
                                 return rc;
                             });
}

// Test hook: the per-op side table of the current programs (plan.hpp ExplainOp), one acl_explain_op_t per FwdOp.  Store-only engines only: it brings the
// HOST snapshot up to date itself, as acl_selfcheck_snapshot does.
int acl_selfcheck_explain_ops(acl_engine_t *h, acl_explain_op_t *out, size_t cap, size_t *n_out) {
    if (!n_out || (cap && !out)) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_selfcheck_explain_ops: bad argument");
    int rc = acl_selfcheck_snapshot(h, nullptr);
    if (rc) return rc;
    std::lock_guard<RwLock> lk(h->state_mu);
    const Snapshot &s = h->snap;
    const std::vector<ExplainOp> x = explain_ops(h->store.schema(), s);
    std::vector<uint32_t> owner(s.ops.size(), 0xFFFFFFFFu);
    for (size_t slot = 0; slot < s.progs.size(); slot++)
        for (uint32_t j = 0; j < s.progs[slot].n_total && s.progs[slot].first + j < owner.size(); j++) owner[s.progs[slot].first + j] = (uint32_t)slot;
    *n_out = x.size();
    for (size_t j = 0; j < x.size() && j < cap; j++) out[j] = acl_explain_op_t{x[j].rtype, x[j].relation, x[j].stype, x[j].srel, owner[j], s.ops[j].dlevel, s.ops[j].flags};
    return ACL_OK;
}

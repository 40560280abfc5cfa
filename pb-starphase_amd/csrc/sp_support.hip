// sp_support.hip -- the host layer of consensus support (no kernel here): the summary rule, the strings of the two lists, ONE support pass that the HLA and the CYP2D6
// cohort drivers both fill and run (SupportPass: sets, anchor, pairs, the device-resident pass of sp_pileup.hip, tables and lists back in the caller's terms), and ONE
// JSON object per consensus that `consensus_support.json` and `cyp2d6_consensus_support.json` are both made of.  Contract: include/starphase_hip.h; design: DESIGN.md
// section 7.2.
#include "sp_internal.h"
#include "sp_json.h"
#include <algorithm>
#include <cstring>
#include <functional>
#include <map>
#include <numeric>

namespace {

bool contested_col(const sp_pileup_col& c) { return pu_contested(c.depth, c.eq, c.ins); }

std::string revcomp_str(const char* s, size_t n) {
    std::string r(n, 'N');
    for (size_t i = 0; i < n; ++i) {
        char c = s[n - 1 - i];
        switch (c) { case 'A': case 'a': c = 'T'; break; case 'C': case 'c': c = 'G'; break; case 'G': case 'g': c = 'C'; break; case 'T': case 't': c = 'A'; break; default: c = 'N'; }
        r[i] = c;
    }
    return r;
}

// a text into the caller's buffer, or how much room it needs
int32_t copy_out(const std::string& text, char* out, uint64_t cap, uint64_t* needed) {
    if (needed) *needed = text.size() + 1;
    if (cap < text.size() + 1) { if (cap) out[0] = '\0'; return SP_ERR_CAPACITY; }
    std::memcpy(out, text.c_str(), text.size() + 1);
    return SP_OK;
}

// the first min(len, 64) bases of a record, from its key
std::string ins_key_string(const sp_pileup_ins& r) {
    std::string out(std::min<uint32_t>(r.len, 64), 'A');
    for (size_t i = 0; i < out.size(); ++i) out[i] = "ACGT"[((i < 32 ? r.p0 >> (2 * i) : r.p1 >> (2 * (i - 32)))) & 3u];
    return out;
}

// ---------------------------------------------------------------------------------------------------------------- the JSON of one consensus
// the lists of a pass as a renderer holds them, and who a record's first_pair is: names[first_pair], or names[mappings[first_pair].read] when mappings is given
struct SupportJsonLists {
    const sp_pileup_ins* ins; uint64_t n_ins; const sp_support_hap* haps; uint64_t n_haps;
    const sp_cyp_read_mapping* mappings; uint64_t n_mappings; const char* const* names; uint32_t n_names;
    // adds "first_read" to a record's object; left out without names or for an index outside them
    void first_read(spj::Value* v, uint64_t who) const {
        bool known = names != nullptr;
        if (known && mappings) { known = who < n_mappings; if (known) who = mappings[who].read; }
        if (known && who < n_names && names[who]) v->obj.emplace_back("first_read", spj::str(names[who]));
    }
};

// adds "insertions" (and "more", "other") to the object of a contested column from the records of column `col` of the list, in record order
void support_ins_json(spj::Value* column, const SupportJsonLists& L, uint64_t col) {
    const sp_pileup_ins* end = L.ins + L.n_ins;
    const sp_pileup_ins* r = std::lower_bound(L.ins, end, col, [](const sp_pileup_ins& a, uint64_t c) { return a.col < c; });
    spj::Value list = spj::array();
    uint64_t more = 0, other = 0;
    for (; r != end && r->col == col; ++r) {
        other += r->n_other;
        if (r->len == 0) continue;
        if (list.arr.size() >= 8) { ++more; continue; }
        spj::Value v = spj::object();
        v.obj.emplace_back("seq", spj::str(ins_key_string(*r))); v.obj.emplace_back("count", spj::unum(r->count));
        if (r->len > 64) v.obj.emplace_back("len", spj::unum(r->len));
        L.first_read(&v, r->first_pair);
        list.arr.push_back(std::move(v));
    }
    column->obj.emplace_back("insertions", std::move(list));
    if (more) column->obj.emplace_back("more", spj::unum(more));
    if (other) column->obj.emplace_back("other", spj::unum(other));
}

// adds "haplotypes" to the object of a consensus (cols: its `length` columns) from the records of target `target` of the list; nothing without a head, or when the
// target's head has n_cols == 0 or no records
void support_hap_json(spj::Value* consensus, const sp_pileup_col* cols, uint32_t length, const SupportJsonLists& L, const sp_support_hap_head* head, uint64_t target) {
    if (!head || head->n_cols == 0 || head->n_records == 0) return;
    const sp_support_hap* end = L.haps + L.n_haps;
    const sp_support_hap* r = std::lower_bound(L.haps, end, target, [](const sp_support_hap& a, uint64_t t) { return a.target < t; });
    if (r == end || r->target != target) return;
    spj::Value v = spj::object(), columns = spj::array(), patterns = spj::array();
    for (uint32_t j = 0; j < length && columns.arr.size() < head->n_cols; ++j) if (contested_col(cols[j])) columns.arr.push_back(spj::unum(j));
    uint64_t more = 0;
    for (; r != end && r->target == target; ++r) {
        if (patterns.arr.size() >= 16) { more += r->count; continue; }
        char text[2 * SP_SUPPORT_HAP_COLS + 1];
        if (sp_support_hap_string(r, text, sizeof text, nullptr) != SP_OK) text[0] = '\0';
        spj::Value p = spj::object();
        p.obj.emplace_back("count", spj::unum(r->count)); p.obj.emplace_back("calls", spj::str(text));
        L.first_read(&p, r->first_pair);
        patterns.arr.push_back(std::move(p));
    }
    v.obj.emplace_back("columns", std::move(columns)); v.obj.emplace_back("columns_total", spj::unum(head->n_cols_total)); v.obj.emplace_back("patterns", std::move(patterns));
    if (more) v.obj.emplace_back("more", spj::unum(more));
    consensus->obj.emplace_back("haplotypes", std::move(v));
}

// the object of one consensus `s` (summary, columns): the summary's numbers, the label (typed_allele or region_type), the contested columns -- each with the insertion
// records of column col_base + pos when its insertions contest it -- and the haplotype records of `target` under `head`
spj::Value consensus_json(const sp_support_summary& sm, const sp_pileup_col* cols, const char* s, const char* label_key, spj::Value label, const SupportJsonLists& L,
                          uint64_t col_base, const sp_support_hap_head* head, uint64_t target) {
    spj::Value v = spj::object();
    v.obj.emplace_back("n_members", spj::unum(sm.n_members)); v.obj.emplace_back("n_aligned", spj::unum(sm.n_aligned)); v.obj.emplace_back("n_unaligned", spj::unum(sm.n_unaligned));
    v.obj.emplace_back("length", spj::unum(sm.length)); v.obj.emplace_back("min_depth", spj::unum(sm.min_depth)); v.obj.emplace_back("median_depth", spj::unum(sm.median_depth));
    v.obj.emplace_back("n_contested", spj::unum(sm.n_contested));
    v.obj.emplace_back(label_key, std::move(label));
    spj::Value list = spj::array();
    for (uint32_t j = 0; j < sm.length; ++j) {
        if (!contested_col(cols[j])) continue;
        spj::Value k = spj::object();
        k.obj.emplace_back("pos", spj::unum(j)); k.obj.emplace_back("depth", spj::unum(cols[j].depth)); k.obj.emplace_back("eq", spj::unum(cols[j].eq));
        spj::Value x = spj::array();
        for (int b = 0; b < 4; ++b) x.arr.push_back(spj::unum(cols[j].x[b]));
        k.obj.emplace_back("x", std::move(x));
        k.obj.emplace_back("del", spj::unum(cols[j].del)); k.obj.emplace_back("ins", spj::unum(cols[j].ins));
        k.obj.emplace_back("consensus_base", spj::str(std::string(1, s[j])));
        if (L.n_ins && 2ull * cols[j].ins > cols[j].depth) support_ins_json(&k, L, col_base + j);
        list.arr.push_back(std::move(k));
    }
    v.obj.emplace_back("contested", std::move(list));
    if (L.n_haps) support_hap_json(&v, cols, sm.length, L, head, target);
    return v;
}

// ---------------------------------------------------------------------------------------------------------------- the support pass
// What the two cohort drivers do differently (DESIGN.md section 7.2 has the table): the text their errors begin with, the names of their two pooled sets, the second
// band, align_pileup_run's own `who`, profile names and way of counting, and three rules --
//   keep_diag      a member without a vote keeps its diagonal in the pair list (it is switched off either way)
//   empty_on_host  no member at all: the summaries are made on the host and nothing is launched (otherwise the pass runs over no pair)
//   cols_required  cols may not be NULL once there are columns, and its room is checked BEFORE `summaries` is cleared (otherwise after, and only when cols is given)
struct SupportRules { const char *who, *set_t, *set_q; int32_t retry_band; const char* pass_who; const char* prof[4]; bool count_attempted, keep_diag, empty_on_host, cols_required; };
// (the HLA pileup launch keeps the profile name it has had in this pass: "pileup")
const SupportRules HLA_RULES = { "consensus support", "csup_t", "csup_q", 256, "consensus support",
                                 { "consensus_support_map", "consensus_support_map_retry", "pileup", "consensus_support_summary" }, true, true, true, true };
const SupportRules CYP_RULES = { "cyp consensus support", "cypsup_t", "cypsup_q", 0, "align_pileup",
                                 { "align_pileup_map", "align_pileup_map_retry", "align_pileup_pile", "align_pileup_summary" }, false, false, false, false };

// One pass over the caller's slots.  A driver hands in, in this order: the lists' arguments (lists), the table's and summaries' arrays (outputs), every slot's target
// sequence or none (slot), then -- behind targets_done -- every member with its target, sequence and the caller's id for it (member: a read for HLA, a mapping record
// for CYP2D6), and runs it.  The targets are the slots that have a sequence, in slot order, so records sorted by target stay sorted in the caller's terms.
struct SupportPass {
    sp_ctx* ctx; const SupportRules& R;
    uint64_t n_slots = 0; uint64_t* col_offset = nullptr; sp_pileup_col* cols = nullptr; uint64_t cols_cap = 0; sp_support_summary* summaries = nullptr;
    sp_pileup_ins* ins = nullptr; uint64_t ins_cap = 0; uint64_t* n_ins = nullptr;
    sp_support_hap* haps = nullptr; uint64_t hap_cap = 0; uint64_t* n_haps = nullptr; sp_support_hap_head* heads = nullptr;
    std::vector<int32_t> target_of;                                           // slot -> target, -1: none
    std::string tblob, qblob; std::vector<uint64_t> toff{0}, qoff{0};         // the targets' and the members' bases; toff is the table's col_offset as well
    std::vector<uint32_t> m_target, members_of; std::vector<uint64_t> m_id;
    // window support (optional): before_pass is called with the target set once it is on the device and fills woff (one entry per target and one more) and wins; the
    // member pass then counts them into wout -- the same pass that makes the table
    std::function<int32_t(const sp_seqset*)> before_pass; std::vector<uint64_t> woff; std::vector<sp_window> wins; std::vector<sp_window_support> wout;

    SupportPass(sp_ctx* c, const SupportRules& r) : ctx(c), R(r) {}
    int32_t fail(int32_t code, const std::string& what) const { return sp_fail(ctx, code, std::string(R.who) + ": " + what); }

    int32_t lists(sp_pileup_ins* ins_, uint64_t ins_cap_, uint64_t* n_ins_, sp_support_hap* haps_, uint64_t hap_cap_, uint64_t* n_haps_, sp_support_hap_head* heads_) {
        if ((ins_ && !n_ins_) || (haps_ && (!n_haps_ || !heads_))) return fail(SP_ERR_INVALID_ARG, "null argument");
        ins = ins_; ins_cap = ins_cap_; n_ins = n_ins_; haps = haps_; hap_cap = hap_cap_; n_haps = n_haps_; heads = heads_;
        if (ins) *n_ins = 0;
        if (haps) *n_haps = 0;
        return SP_OK;
    }
    void outputs(uint64_t n_slots_, uint64_t* col_offset_, sp_pileup_col* cols_, uint64_t cols_cap_, sp_support_summary* summaries_) {
        n_slots = n_slots_; col_offset = col_offset_; cols = cols_; cols_cap = cols_cap_; summaries = summaries_;
        col_offset[0] = 0;
    }
    // the next slot: its target sequence on the strand the members are on, len 0: none
    void slot(const char* s, size_t len) {
        const size_t x = target_of.size();
        col_offset[x + 1] = col_offset[x] + len;
        target_of.push_back(len ? (int32_t)(toff.size() - 1) : -1);
        if (len) { tblob.append(s, len); toff.push_back(tblob.size()); }
    }
    // every slot is in: the table's room, the summaries cleared.  *done: no slot has a target, and everything is returned already
    int32_t targets_done(bool* done) {
        const uint64_t n_cols = col_offset[n_slots];
        if (!R.cols_required) std::memset(summaries, 0, sizeof(sp_support_summary) * n_slots);
        if (R.cols_required ? (n_cols > cols_cap || (n_cols && !cols)) : (cols && n_cols > cols_cap))
            return fail(SP_ERR_CAPACITY, std::to_string(n_cols) + " columns, room for " + std::to_string(cols ? cols_cap : 0));
        if (R.cols_required) std::memset(summaries, 0, sizeof(sp_support_summary) * n_slots);
        *done = toff.size() == 1;
        if (*done && haps) std::memset(heads, 0, sizeof(sp_support_hap_head) * n_slots);
        members_of.assign(toff.size() - 1, 0);
        return SP_OK;
    }
    void member(int32_t target, const char* s, size_t len, uint64_t id) {
        qblob.append(s, len); qoff.push_back(qblob.size());
        m_target.push_back((uint32_t)target); m_id.push_back(id); ++members_of[target];
    }

    // The two sets, one anchor launch for the diagonals, every member a pair of ONE device-resident pass (align_pileup_run: 64 diagonals, then R.retry_band for the
    // attempted pairs that came back with score 0 or without ops; no op row reaches the host).  A member without a vote stays in the list switched off, so it counts
    // as unaligned.  Then everything back in the caller's terms.  A list that did not fit: SP_ERR_CAPACITY, and everything else is complete, the other list included.
    int32_t run() {
        const uint32_t n_t = (uint32_t)toff.size() - 1, n_m = (uint32_t)m_target.size();
        sp_seqset T, Q;
        int32_t rc = sp_seqset_make_small(ctx, R.set_t, tblob.data(), toff.data(), n_t, true, &T);
        if (rc != SP_OK) return rc;
        if (before_pass) { rc = before_pass(&T); if (rc != SP_OK) return rc; }
        wout.assign(wins.size(), sp_window_support{});
        const WinIn wi = { woff.data(), wins.data(), wout.data() };
        std::vector<sp_pair> pairs(n_m);
        if (n_m) {
            rc = sp_seqset_make_small(ctx, R.set_q, qblob.data(), qoff.data(), n_m, false, &Q);
            if (rc != SP_OK) return rc;
            std::vector<uint32_t> ident(n_m); std::iota(ident.begin(), ident.end(), 0u);
            std::vector<int32_t> diag(n_m), votes(n_m);
            rc = sp_anchor_batch(ctx, &T, &Q, m_target.data(), ident.data(), n_m, diag.data(), votes.data());
            if (rc != SP_OK) return rc;
            for (uint32_t m = 0; m < n_m; ++m) pairs[m] = sp_pair{ m, m_target[m], (votes[m] > 0 || R.keep_diag) ? -diag[m] : 0, votes[m] > 0 ? 0 : -1 };
        } else { Q = sp_seqset(); Q.ctx = ctx; }
        std::vector<sp_pileup_col> table(cols ? col_offset[n_slots] : 0);
        std::vector<sp_support_summary> sums(n_t);
        std::vector<sp_support_hap_head> t_heads(haps ? n_t : 0);
        if (n_m || !R.empty_on_host) {
            const sp_affine_opts ao = { 1, 4, 6, 2, 26, 1, 1 };
            const HapOut ho = { haps, hap_cap, n_haps, t_heads.data() };
            rc = align_pileup_run(ctx, &Q, &T, pairs.data(), n_m, &ao, 64, R.retry_band, toff.data(), nullptr, cols ? table.data() : nullptr, sums.data(), members_of.data(), nullptr,
                                  R.pass_who, R.prof, R.count_attempted, ins, ins_cap, n_ins, 0, haps ? &ho : nullptr, wins.empty() ? nullptr : &wi);
            if (rc != SP_OK && !(rc == SP_ERR_CAPACITY && ((ins && *n_ins > ins_cap) || (haps && *n_haps > hap_cap)))) return rc;
        } else for (uint32_t t = 0; t < n_t; ++t) sp_support_summarize(table.data() + toff[t], (uint32_t)(toff[t + 1] - toff[t]), 0, 0, &sums[t]);
        for (uint64_t x = 0; x < n_slots; ++x) {
            const int32_t t = target_of[x];
            if (t < 0) continue;
            summaries[x] = sums[t];
            if (cols) std::memcpy(cols + col_offset[x], table.data() + toff[t], sizeof(sp_pileup_col) * (size_t)(toff[t + 1] - toff[t]));
        }
        if (ins && *n_ins && *n_ins <= ins_cap) {
            // the insertion list in the caller's terms: col in col_offset's space, first_pair the member's id
            std::vector<uint64_t> base(n_t, 0);
            for (uint64_t x = 0; x < n_slots; ++x) if (target_of[x] >= 0) base[target_of[x]] = col_offset[x];
            for (uint64_t k = 0; k < *n_ins; ++k) {
                const uint32_t t = (uint32_t)(std::upper_bound(toff.begin(), toff.end(), ins[k].col) - toff.begin()) - 1;
                ins[k].col = base[t] + (ins[k].col - toff[t]);
                if (ins[k].len) ins[k].first_pair = (uint32_t)m_id[ins[k].first_pair];
            }
        }
        if (haps && *n_haps <= hap_cap) {
            // the haplotype list in the caller's terms: target = the slot, first_pair = the member's id; a slot without a target has an empty head at the running record
            std::vector<uint64_t> slot_of(n_t, 0);
            uint64_t at = 0;
            for (uint64_t x = 0; x < n_slots; ++x) {
                const int32_t t = target_of[x];
                if (t >= 0) { slot_of[t] = x; heads[x] = t_heads[t]; at = t_heads[t].first_record + t_heads[t].n_records; }
                else { heads[x] = sp_support_hap_head{}; heads[x].first_record = at; }
            }
            for (uint64_t k = 0; k < *n_haps; ++k) { haps[k].target = slot_of[haps[k].target]; haps[k].first_pair = (uint32_t)m_id[haps[k].first_pair]; }
        }
        return rc;
    }
};

int32_t cyp_support_cohort_fill(SupportPass& P, sp_ctx* ctx, uint32_t n_samples, const sp_seqset* const* reads, const sp_cyp_call* calls, const char* consensus, uint32_t cons_cap,
                                const sp_cyp_read_mapping* mappings, const uint64_t* mapping_off, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap,
                                sp_support_summary* summaries, sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins,
                                sp_support_hap* haps, uint64_t hap_cap, uint64_t* n_haps, sp_support_hap_head* heads);      // (the CYP2D6 drivers' slots and members; below)

// a single call's status behind its cohort form: a list that did not fit still leaves everything else to hand on
bool only_a_list_short(int32_t rc, const sp_pileup_ins* ins, const uint64_t* n_ins, uint64_t ins_cap, const sp_support_hap* haps, const uint64_t* n_haps, uint64_t hap_cap) {
    return rc == SP_ERR_CAPACITY && ((ins && n_ins && *n_ins > ins_cap) || (haps && n_haps && *n_haps > hap_cap));
}

} // namespace

extern "C" {

int32_t sp_support_ins_string(const sp_pileup_ins* rec, const sp_seqset* queries, uint32_t query, char* out, uint64_t cap, uint64_t* needed) {
    if (!rec || (cap && !out)) return SP_ERR_INVALID_ARG;
    std::string text;
    if (rec->len <= 64) text = ins_key_string(*rec);
    else {
        if (!queries || !queries->ctx || query >= queries->n || (uint64_t)rec->first_qpos + rec->len > (uint64_t)queries->h_len[query]) return SP_ERR_INVALID_ARG;
        const std::string whole = sp_seqset_decode(queries->ctx, queries, query);
        if ((int32_t)whole.size() != queries->h_len[query]) return SP_ERR_HIP;
        text = whole.substr(rec->first_qpos, rec->len);
    }
    return copy_out(text, out, cap, needed);
}

int32_t sp_support_hap_string(const sp_support_hap* rec, char* out, uint64_t cap, uint64_t* needed) {
    if (!rec || (cap && !out) || rec->n_cols > SP_SUPPORT_HAP_COLS) return SP_ERR_INVALID_ARG;
    std::string text;
    for (uint32_t k = 0; k < rec->n_cols; ++k) {
        const uint32_t call = (uint32_t)(rec->w[k >> 4] >> ((k & 15) << 2)) & 15u;
        text += "?=ACGT-?"[call & 7u];
        if (call & 8u) text += '+';
    }
    return copy_out(text, out, cap, needed);
}

int32_t sp_support_summarize(const sp_pileup_col* cols, uint32_t length, uint32_t n_members, uint32_t n_aligned, sp_support_summary* out) {
    if (!out || (length && !cols) || n_aligned > n_members) return SP_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof *out);
    out->n_members = n_members; out->n_aligned = n_aligned; out->n_unaligned = n_members - n_aligned; out->length = length;
    if (length == 0) return SP_OK;
    std::vector<uint32_t> depth(length);
    for (uint32_t j = 0; j < length; ++j) { depth[j] = cols[j].depth; if (contested_col(cols[j])) ++out->n_contested; }
    std::nth_element(depth.begin(), depth.begin() + (length - 1) / 2, depth.end());
    out->median_depth = depth[(length - 1) / 2];
    out->min_depth = *std::min_element(depth.begin(), depth.end());
    return SP_OK;
}

int32_t sp_support_contested(const sp_pileup_col* cols, uint32_t length, uint32_t* pos, uint32_t cap, uint32_t* n) {
    if (!n || (length && !cols) || (cap && !pos)) return SP_ERR_INVALID_ARG;
    uint32_t k = 0;
    for (uint32_t j = 0; j < length; ++j) if (contested_col(cols[j])) { if (k < cap) pos[k] = j; ++k; }
    *n = k;
    return k > cap ? SP_ERR_CAPACITY : SP_OK;
}

// ---------------------------------------------------------------------------------------------------------------- consensus_support.json
int32_t sp_consensus_support_json(const sp_support_entry* entries, uint32_t n_entries, char* out, uint64_t cap, uint64_t* needed) {
    return sp_consensus_support_json_ins(entries, n_entries, nullptr, nullptr, 0, nullptr, 0, out, cap, needed);
}

int32_t sp_consensus_support_json_ins(const sp_support_entry* entries, uint32_t n_entries, const uint64_t* col_base, const sp_pileup_ins* ins, uint64_t n_ins,
                                      const char* const* read_names, uint32_t n_read_names, char* out, uint64_t cap, uint64_t* needed) {
    return sp_consensus_support_json_hap(entries, n_entries, col_base, ins, n_ins, nullptr, 0, nullptr, 0, nullptr, read_names, n_read_names, out, cap, needed);
}

int32_t sp_consensus_support_json_hap(const sp_support_entry* entries, uint32_t n_entries, const uint64_t* col_base, const sp_pileup_ins* ins, uint64_t n_ins,
                                      const sp_support_hap* haps, uint64_t n_haps, const sp_support_hap_head* heads, uint64_t n_heads, const uint64_t* hap_target,
                                      const char* const* read_names, uint32_t n_read_names, char* out, uint64_t cap, uint64_t* needed) {
    if (n_haps && (!haps || !heads || (n_entries && !hap_target))) return SP_ERR_INVALID_ARG;
    if ((n_entries && !entries) || (cap && !out) || (n_ins && !ins) || (n_entries && n_ins && !col_base)) return SP_ERR_INVALID_ARG;     // (without entries no col_base is read)
    std::vector<uint32_t> order;
    for (uint32_t e = 0; e < n_entries; ++e) {
        if (!entries[e].gene) return SP_ERR_INVALID_ARG;
        for (int c = 0; c < 2; ++c) {
            const char* s = entries[e].consensus[c];
            if (!s || !*s) continue;
            if (!entries[e].summary[c] || !entries[e].cols[c] || std::strlen(s) != entries[e].summary[c]->length) return SP_ERR_INVALID_ARG;
        }
        order.push_back(e);
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return std::strcmp(entries[a].gene, entries[b].gene) < 0; });
    const SupportJsonLists L = { ins, n_ins, haps, n_haps, nullptr, 0, read_names, n_read_names };
    spj::Value root = spj::object();
    for (size_t o = 0; o < order.size(); ++o) {
        const sp_support_entry& en = entries[order[o]];
        if (o && std::strcmp(entries[order[o - 1]].gene, en.gene) == 0) return SP_ERR_INVALID_ARG;      // one entry per gene
        spj::Value gene = spj::object();
        for (int c = 0; c < 2; ++c) {
            const char* s = en.consensus[c];
            if (!s || !*s) continue;
            const size_t x = 2 * (size_t)order[o] + c;
            const uint64_t target = n_haps ? hap_target[x] : 0;
            gene.obj.emplace_back(c ? "consensus2" : "consensus1",
                                  consensus_json(*en.summary[c], en.cols[c], s, "typed_allele", en.typed_allele[c] ? spj::str(en.typed_allele[c]) : spj::Value(), L,
                                                 n_ins ? col_base[x] : 0, n_haps && target < n_heads ? heads + target : nullptr, target));
        }
        if (!gene.obj.empty()) root.obj.emplace_back(en.gene, std::move(gene));
    }
    std::string text;
    spj::write_pretty(text, root);
    return copy_out(text, out, cap, needed);
}

// ---------------------------------------------------------------------------------------------------------------- HLA consensus support
// The driver's own: the gene table and its duplicate check, strands (targets and members go onto the gene strand), unit_on, members read from sp_hla_realign.
int32_t sp_hla_consensus_support_cohort_hap(sp_ctx* ctx, const sp_hla_db* db, uint32_t n_samples, const uint32_t* read_sample, uint32_t n_genes, const uint32_t* genes,
                                            const sp_seqset* reads, const sp_hla_realign* realign, const uint8_t* is_cons1, const char* cons, uint32_t cap,
                                            const uint8_t* unit_on, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap, sp_support_summary* summaries,
                                            sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins,
                                            sp_support_hap* haps, uint64_t hap_cap, uint64_t* n_haps, sp_support_hap_head* heads) {
    if (!ctx) return SP_ERR_INVALID_ARG;
    SupportPass P(ctx, HLA_RULES);
    int32_t rc = P.lists(ins, ins_cap, n_ins, haps, hap_cap, n_haps, heads);
    if (rc != SP_OK) return rc;
    if (!db || !reads || !col_offset || !summaries || n_samples == 0 || (n_genes && (!genes || !cons || cap == 0)) || (reads->n && (!realign || !is_cons1)) || (n_samples > 1 && !read_sample))
        return P.fail(SP_ERR_INVALID_ARG, "null argument");
    const uint64_t n_units = (uint64_t)n_samples * n_genes;
    std::map<uint32_t, uint32_t> gene_slot;                                   // gene -> its place in `genes`
    for (uint32_t k = 0; k < n_genes; ++k) {
        if (spi_hla_gene_fwd(db, genes[k]) < 0) return P.fail(SP_ERR_INVALID_ARG, "gene out of range");
        if (!gene_slot.emplace(genes[k], k).second) return P.fail(SP_ERR_INVALID_ARG, "a gene is listed twice");
    }
    // ---- the slots: the two consensuses of every unit; a target is a non-empty consensus of a unit that is on
    P.outputs(2 * n_units, col_offset, cols, cols_cap, summaries);
    for (uint64_t u = 0; u < n_units; ++u) for (int c = 0; c < 2; ++c) {
        const char* s = cons + (2 * u + c) * (size_t)cap;
        const size_t len = (unit_on && !unit_on[u]) ? 0 : strnlen(s, cap);
        if (len == 0 || spi_hla_gene_fwd(db, genes[u % n_genes])) P.slot(s, len); else P.slot(revcomp_str(s, len).data(), len);
    }
    bool done = false;
    rc = P.targets_done(&done);
    if (rc != SP_OK || done) return rc;
    // ---- the members: the realigned reads of every unit whose group has a consensus
    for (uint32_t r = 0; r < reads->n; ++r) {
        const sp_hla_realign& q = realign[r];
        if (q.status != 0 || q.gene < 0) continue;
        const auto slot = gene_slot.find((uint32_t)q.gene);
        if (slot == gene_slot.end()) continue;
        const uint32_t sample = read_sample ? read_sample[r] : 0;
        if (sample >= n_samples) return P.fail(SP_ERR_INVALID_ARG, "read_sample out of range");
        const int32_t t = P.target_of[2 * ((uint64_t)sample * n_genes + slot->second) + (is_cons1[r] ? 0 : 1)];
        if (t < 0) continue;
        if (q.seg_start < 0 || q.seg_end <= q.seg_start || q.seg_end > reads->h_len[r]) return P.fail(SP_ERR_INVALID_ARG, "segment outside its read");
        const std::string whole = sp_seqset_decode(ctx, reads, r);
        if ((int32_t)whole.size() != reads->h_len[r]) return P.fail(SP_ERR_HIP, "fetching the reads failed");
        const size_t len = (size_t)(q.seg_end - q.seg_start);
        if (spi_hla_gene_fwd(db, (uint32_t)q.gene)) P.member(t, whole.data() + q.seg_start, len, r); else P.member(t, revcomp_str(whole.data() + q.seg_start, len).data(), len, r);
    }
    return P.run();
}

// the entries without one list or both: the same path, the list's arguments NULL
int32_t sp_hla_consensus_support_cohort_ins(sp_ctx* ctx, const sp_hla_db* db, uint32_t n_samples, const uint32_t* read_sample, uint32_t n_genes, const uint32_t* genes,
                                            const sp_seqset* reads, const sp_hla_realign* realign, const uint8_t* is_cons1, const char* cons, uint32_t cap,
                                            const uint8_t* unit_on, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap, sp_support_summary* summaries,
                                            sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins) {
    return sp_hla_consensus_support_cohort_hap(ctx, db, n_samples, read_sample, n_genes, genes, reads, realign, is_cons1, cons, cap, unit_on, col_offset, cols, cols_cap, summaries,
                                               ins, ins_cap, n_ins, nullptr, 0, nullptr, nullptr);
}

int32_t sp_hla_consensus_support_cohort(sp_ctx* ctx, const sp_hla_db* db, uint32_t n_samples, const uint32_t* read_sample, uint32_t n_genes, const uint32_t* genes,
                                        const sp_seqset* reads, const sp_hla_realign* realign, const uint8_t* is_cons1, const char* cons, uint32_t cap,
                                        const uint8_t* unit_on, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap, sp_support_summary* summaries) {
    return sp_hla_consensus_support_cohort_ins(ctx, db, n_samples, read_sample, n_genes, genes, reads, realign, is_cons1, cons, cap, unit_on, col_offset, cols, cols_cap, summaries, nullptr, 0, nullptr);
}

// one gene call: the cohort form over one sample and one gene
int32_t sp_hla_consensus_support_hap(sp_ctx* ctx, const sp_hla_db* db, uint32_t gene, const sp_seqset* reads, const sp_hla_realign* realign, const uint8_t* is_cons1,
                                     const char* cons1, const char* cons2, sp_pileup_col* cols1, sp_pileup_col* cols2, sp_support_summary* s1, sp_support_summary* s2,
                                     sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins, sp_support_hap* haps, uint64_t hap_cap, uint64_t* n_haps, sp_support_hap_head* heads) {
    if (!ctx) return SP_ERR_INVALID_ARG;
    if (!cons1 || !cons2) return sp_fail(ctx, SP_ERR_INVALID_ARG, "consensus support: null argument");
    const size_t l1 = cols1 && s1 ? std::strlen(cons1) : 0, l2 = cols2 && s2 ? std::strlen(cons2) : 0;
    const uint32_t cap = (uint32_t)std::max(l1, l2) + 1;
    std::vector<char> both((size_t)2 * cap, '\0');
    std::memcpy(both.data(), cons1, l1); std::memcpy(both.data() + cap, cons2, l2);
    uint64_t off[3]; sp_support_summary sm[2];
    std::vector<sp_pileup_col> table(l1 + l2);
    const int32_t rc = sp_hla_consensus_support_cohort_hap(ctx, db, 1, nullptr, 1, &gene, reads, realign, is_cons1, both.data(), cap, nullptr, off, table.data(), table.size(), sm, ins, ins_cap, n_ins,
                                                           haps, hap_cap, n_haps, heads);
    if (rc != SP_OK && !only_a_list_short(rc, ins, n_ins, ins_cap, haps, n_haps, hap_cap)) return rc;
    if (cols1 && s1) { std::memcpy(cols1, table.data(), sizeof(sp_pileup_col) * l1); *s1 = sm[0]; }
    if (cols2 && s2) { std::memcpy(cols2, table.data() + off[1], sizeof(sp_pileup_col) * l2); *s2 = sm[1]; }
    return rc;
}

int32_t sp_hla_consensus_support_ins(sp_ctx* ctx, const sp_hla_db* db, uint32_t gene, const sp_seqset* reads, const sp_hla_realign* realign, const uint8_t* is_cons1,
                                     const char* cons1, const char* cons2, sp_pileup_col* cols1, sp_pileup_col* cols2, sp_support_summary* s1, sp_support_summary* s2,
                                     sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins) {
    return sp_hla_consensus_support_hap(ctx, db, gene, reads, realign, is_cons1, cons1, cons2, cols1, cols2, s1, s2, ins, ins_cap, n_ins, nullptr, 0, nullptr, nullptr);
}

int32_t sp_hla_consensus_support(sp_ctx* ctx, const sp_hla_db* db, uint32_t gene, const sp_seqset* reads, const sp_hla_realign* realign, const uint8_t* is_cons1,
                                 const char* cons1, const char* cons2, sp_pileup_col* cols1, sp_pileup_col* cols2, sp_support_summary* s1, sp_support_summary* s2) {
    return sp_hla_consensus_support_ins(ctx, db, gene, reads, realign, is_cons1, cons1, cons2, cols1, cols2, s1, s2, nullptr, 0, nullptr);
}

// ---------------------------------------------------------------------------------------------------------------- CYP2D6 consensus support
// The driver's own: slots from calls[i].status / n_consensus (a call that failed owns none), members read from sp_cyp_read_mapping, a read with several regions fetched
// once per sample.  The members' segments are forward views of the reads as uploaded and the consensuses were built from such segments (the parts of sp_cyp.hip cut
// every region with sp_make_segments, which has no strand; sp_region_hit carries none): one orientation, no strand handling.
} // extern "C"

// The cohort pass with everything it can make (declared in sp_internal.h for the whole-sample call).  vin (optional): the variant support of sp_cyp_variant_support_cohort --
// the windows of the database variants on every typed region, counted by the SAME member pass that makes the table.
int32_t spi_cyp_support_cohort(sp_ctx* ctx, uint32_t n_samples, const sp_seqset* const* reads, const sp_cyp_call* calls, const char* consensus, uint32_t cons_cap,
                               const sp_cyp_read_mapping* mappings, const uint64_t* mapping_off, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap,
                               sp_support_summary* summaries, sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins,
                               sp_support_hap* haps, uint64_t hap_cap, uint64_t* n_haps, sp_support_hap_head* heads, const CypVariantIn* vin) {
    if (!ctx) return SP_ERR_INVALID_ARG;
    SupportPass P(ctx, CYP_RULES);
    std::vector<uint64_t> win_at;                                        // window -> its place in vin->support
    if (vin) {
        if (!vin->problem || !vin->rv || !vin->support || !vin->valid || n_samples == 0) return P.fail(SP_ERR_INVALID_ARG, "null argument");
        const size_t total = (size_t)n_samples * SP_CYP_MAXCONS * vin->problem->n_variants;
        std::memset(vin->support, 0, sizeof(sp_window_support) * total);
        std::memset(vin->valid, 0, sizeof(int32_t) * total);
        // every typed consensus onto the backbone: one anchor launch for the diagonals, one affine alignment at the map-hifi scores on 256 diagonals; then the rule
        // of sp_cyp_variant_windows
        P.before_pass = [&P, &win_at, vin, ctx](const sp_seqset* T) -> int32_t {
            const sp_cyp_problem* pr = vin->problem;
            const uint32_t NV = pr->n_variants;
            P.woff.assign((size_t)T->n + 1, 0);
            std::vector<uint32_t> tt; std::vector<uint64_t> slot;
            for (uint64_t x = 0; x < P.n_slots; ++x) if (P.target_of[x] >= 0 && vin->rv[x / SP_CYP_MAXCONS].has_variants[x % SP_CYP_MAXCONS] == 1) { tt.push_back((uint32_t)P.target_of[x]); slot.push_back(x); }
            if (tt.empty() || NV == 0) return SP_OK;
            if (!pr->backbone || !pr->var_pos || !pr->var_ref) return P.fail(SP_ERR_INVALID_ARG, "null argument");
            const uint32_t n = (uint32_t)tt.size(), stride = 4096;
            const uint64_t boff[2] = { 0, pr->backbone_len };
            sp_seqset BB;
            int32_t rc = sp_seqset_make_small(ctx, "cypvar_bb", pr->backbone, boff, 1, false, &BB);
            if (rc != SP_OK) return rc;
            std::vector<uint32_t> zero(n, 0), n_cigar(n), cigar((size_t)n * stride), ref_len(NV);
            std::vector<int32_t> diag(n), votes(n), ok(NV);
            rc = sp_anchor_batch(ctx, T, &BB, tt.data(), zero.data(), n, diag.data(), votes.data());
            if (rc != SP_OK) return rc;
            std::vector<sp_pair> bp(n);
            for (uint32_t k = 0; k < n; ++k) bp[k] = sp_pair{ tt[k], 0, votes[k] > 0 ? diag[k] : 0, votes[k] > 0 ? 0 : -1 };
            std::vector<sp_affine_aln> aln(n);
            const sp_affine_opts ao = { 1, 4, 6, 2, 26, 1, 1 };
            rc = sp_affine_align_batch(ctx, T, &BB, bp.data(), n, &ao, 256, aln.data(), cigar.data(), stride, n_cigar.data());
            if (rc != SP_OK) return rc;
            for (uint32_t v = 0; v < NV; ++v) ref_len[v] = (uint32_t)std::strlen(pr->var_ref[v]);
            std::vector<sp_window> w(NV);
            for (uint32_t k = 0; k < n; ++k) {                             // (tt ascends with the slots: the windows come out in target order)
                if (n_cigar[k] == 0 || n_cigar[k] > stride) continue;        // no alignment onto the backbone (or one of more runs than a row keeps): no windows, SR and CR stay '.'
                rc = sp_cyp_variant_windows(&aln[k], cigar.data() + (size_t)k * stride, n_cigar[k], NV, pr->var_pos, ref_len.data(), vin->flank, w.data(), ok.data());
                if (rc != SP_OK) return P.fail(rc, "the alignment onto the backbone does not consume its spans");
                for (uint32_t v = 0; v < NV; ++v) if (ok[v]) { P.wins.push_back(w[v]); win_at.push_back(slot[k] * NV + v); ++P.woff[(size_t)tt[k] + 1]; }
            }
            for (uint32_t t = 0; t < T->n; ++t) P.woff[t + 1] += P.woff[t];
            return SP_OK;
        };
    }
    const int32_t rc_pass = cyp_support_cohort_fill(P, ctx, n_samples, reads, calls, consensus, cons_cap, mappings, mapping_off, col_offset, cols, cols_cap, summaries, ins, ins_cap, n_ins,
                                                    haps, hap_cap, n_haps, heads);
    if (vin && (rc_pass == SP_OK || rc_pass == SP_ERR_CAPACITY) && P.wout.size() == win_at.size())
        for (size_t j = 0; j < win_at.size(); ++j) { vin->support[win_at[j]] = P.wout[j]; vin->valid[win_at[j]] = 1; }
    return rc_pass;
}

extern "C" {

int32_t sp_cyp_consensus_support_cohort_hap(sp_ctx* ctx, uint32_t n_samples, const sp_seqset* const* reads, const sp_cyp_call* calls, const char* consensus, uint32_t cons_cap,
                                            const sp_cyp_read_mapping* mappings, const uint64_t* mapping_off, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap,
                                            sp_support_summary* summaries, sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins,
                                            sp_support_hap* haps, uint64_t hap_cap, uint64_t* n_haps, sp_support_hap_head* heads) {
    return spi_cyp_support_cohort(ctx, n_samples, reads, calls, consensus, cons_cap, mappings, mapping_off, col_offset, cols, cols_cap, summaries, ins, ins_cap, n_ins, haps, hap_cap, n_haps, heads, nullptr);
}

// the variant support of a cohort: the pass above with the windows attached; the table's outputs are optional (col_offset == NULL: only support / support_valid are made)
int32_t sp_cyp_variant_support_cohort(sp_ctx* ctx, const sp_cyp_problem* problem, uint32_t n_samples, const sp_seqset* const* reads, const sp_cyp_call* calls, const char* consensus,
                                      uint32_t cons_cap, const sp_cyp_region_variants* region_variants, const sp_cyp_read_mapping* mappings, const uint64_t* mapping_off, uint32_t flank,
                                      sp_window_support* support, int32_t* support_valid, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap, sp_support_summary* summaries) {
    if (!ctx) return SP_ERR_INVALID_ARG;
    if (!problem || !region_variants || !support || !support_valid || n_samples == 0) return sp_fail(ctx, SP_ERR_INVALID_ARG, "cyp variant support: null argument");
    std::vector<uint64_t> off(col_offset ? 0 : (size_t)n_samples * SP_CYP_MAXCONS + 1);
    std::vector<sp_support_summary> sm(summaries ? 0 : (size_t)n_samples * SP_CYP_MAXCONS);
    const CypVariantIn vin = { problem, region_variants, flank, support, support_valid };
    return spi_cyp_support_cohort(ctx, n_samples, reads, calls, consensus, cons_cap, mappings, mapping_off, col_offset ? col_offset : off.data(), col_offset ? cols : nullptr, col_offset ? cols_cap : 0,
                                  summaries ? summaries : sm.data(), nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, &vin);
}

int32_t sp_cyp_variant_support(sp_ctx* ctx, const sp_cyp_problem* problem, const sp_seqset* reads, const sp_cyp_call* call, const char* consensus, uint32_t cons_cap,
                               const sp_cyp_region_variants* region_variants, const sp_cyp_read_mapping* mappings, uint64_t n_mappings, uint32_t flank,
                               sp_window_support* support, int32_t* support_valid, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap, sp_support_summary* summaries) {
    if (!ctx) return SP_ERR_INVALID_ARG;
    if (!call) return sp_fail(ctx, SP_ERR_INVALID_ARG, "cyp variant support: null argument");
    const int32_t H = std::min<int32_t>(std::max<int32_t>(call->n_consensus, 0), SP_CYP_MAXCONS);
    uint64_t off[SP_CYP_MAXCONS + 1] = { 0 }; sp_support_summary sm[SP_CYP_MAXCONS];
    const uint64_t moff[2] = { 0, n_mappings };
    const int32_t rc = sp_cyp_variant_support_cohort(ctx, problem, 1, &reads, call, consensus, cons_cap, region_variants, mappings, moff, flank, support, support_valid,
                                                     col_offset ? off : nullptr, cols, cols_cap, col_offset ? sm : nullptr);
    if (col_offset) std::memcpy(col_offset, off, sizeof(uint64_t) * ((size_t)H + 1));
    if (rc == SP_OK && col_offset && summaries) std::memcpy(summaries, sm, sizeof(sp_support_summary) * (size_t)H);
    return rc;
}

} // extern "C"

namespace {
// the member pass of the CYP2D6 drivers: lists, slots, members, run
int32_t cyp_support_cohort_fill(SupportPass& P, sp_ctx* ctx, uint32_t n_samples, const sp_seqset* const* reads, const sp_cyp_call* calls, const char* consensus, uint32_t cons_cap,
                                const sp_cyp_read_mapping* mappings, const uint64_t* mapping_off, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap,
                                sp_support_summary* summaries, sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins,
                                sp_support_hap* haps, uint64_t hap_cap, uint64_t* n_haps, sp_support_hap_head* heads) {
    int32_t rc = P.lists(ins, ins_cap, n_ins, haps, hap_cap, n_haps, heads);
    if (rc != SP_OK) return rc;
    if (!reads || !calls || !mapping_off || !col_offset || !summaries || n_samples == 0) return P.fail(SP_ERR_INVALID_ARG, "null argument");
    // ---- the slots: SP_CYP_MAXCONS per sample; a target is a non-empty consensus of a call that succeeded, as the call returned it
    P.outputs((uint64_t)n_samples * SP_CYP_MAXCONS, col_offset, cols, cols_cap, summaries);
    for (uint32_t i = 0; i < n_samples; ++i) {
        const int32_t H = calls[i].status == 0 ? std::min<int32_t>(std::max<int32_t>(calls[i].n_consensus, 0), SP_CYP_MAXCONS) : 0;
        if (H > 0 && (!consensus || cons_cap == 0 || !reads[i])) return P.fail(SP_ERR_INVALID_ARG, "null argument");
        for (int32_t h = 0; h < SP_CYP_MAXCONS; ++h) {
            const char* s = h < H ? consensus + ((uint64_t)i * SP_CYP_MAXCONS + h) * (size_t)cons_cap : nullptr;
            P.slot(s, s ? strnlen(s, cons_cap) : 0);
        }
    }
    bool done = false;
    rc = P.targets_done(&done);
    if (rc != SP_OK || done) return rc;
    // ---- the members: one per mapping record whose consensus is a target
    for (uint32_t i = 0; i < n_samples; ++i) {
        if (calls[i].status != 0 || mapping_off[i + 1] == mapping_off[i]) continue;
        if (mapping_off[i + 1] < mapping_off[i] || !mappings || !reads[i]) return P.fail(SP_ERR_INVALID_ARG, "mapping_off");
        std::map<uint32_t, std::string> decoded;                         // (a read with several regions is fetched once)
        for (uint64_t k = mapping_off[i]; k < mapping_off[i + 1]; ++k) {
            const sp_cyp_read_mapping& q = mappings[k];
            if (q.consensus >= (uint32_t)SP_CYP_MAXCONS || q.read >= reads[i]->n) return P.fail(SP_ERR_INVALID_ARG, "mapping out of range");
            const int32_t t = P.target_of[(uint64_t)i * SP_CYP_MAXCONS + q.consensus];
            if (t < 0) continue;
            if (q.read_end <= q.read_start || q.read_end > (uint64_t)reads[i]->h_len[q.read]) return P.fail(SP_ERR_INVALID_ARG, "segment outside its read");
            auto it = decoded.find(q.read);
            if (it == decoded.end()) {
                it = decoded.emplace(q.read, sp_seqset_decode(ctx, reads[i], q.read)).first;
                if ((int32_t)it->second.size() != reads[i]->h_len[q.read]) return P.fail(SP_ERR_HIP, "fetching the reads failed");
            }
            P.member(t, it->second.data() + q.read_start, (size_t)(q.read_end - q.read_start), k);
        }
    }
    return P.run();
}
} // namespace
extern "C" {

int32_t sp_cyp_consensus_support_cohort_ins(sp_ctx* ctx, uint32_t n_samples, const sp_seqset* const* reads, const sp_cyp_call* calls, const char* consensus, uint32_t cons_cap,
                                            const sp_cyp_read_mapping* mappings, const uint64_t* mapping_off, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap,
                                            sp_support_summary* summaries, sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins) {
    return sp_cyp_consensus_support_cohort_hap(ctx, n_samples, reads, calls, consensus, cons_cap, mappings, mapping_off, col_offset, cols, cols_cap, summaries, ins, ins_cap, n_ins,
                                               nullptr, 0, nullptr, nullptr);
}

int32_t sp_cyp_consensus_support_cohort(sp_ctx* ctx, uint32_t n_samples, const sp_seqset* const* reads, const sp_cyp_call* calls, const char* consensus, uint32_t cons_cap,
                                        const sp_cyp_read_mapping* mappings, const uint64_t* mapping_off, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap,
                                        sp_support_summary* summaries) {
    return sp_cyp_consensus_support_cohort_ins(ctx, n_samples, reads, calls, consensus, cons_cap, mappings, mapping_off, col_offset, cols, cols_cap, summaries, nullptr, 0, nullptr);
}

// one sample: the cohort form over it
int32_t sp_cyp_consensus_support_hap(sp_ctx* ctx, const sp_seqset* reads, const sp_cyp_call* call, const char* consensus, uint32_t cons_cap,
                                     const sp_cyp_read_mapping* mappings, uint64_t n_mappings, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap,
                                     sp_support_summary* summaries, sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins,
                                     sp_support_hap* haps, uint64_t hap_cap, uint64_t* n_haps, sp_support_hap_head* heads) {
    if (!ctx) return SP_ERR_INVALID_ARG;
    if (!call || !col_offset || !summaries) return sp_fail(ctx, SP_ERR_INVALID_ARG, "cyp consensus support: null argument");
    const int32_t H = std::min<int32_t>(std::max<int32_t>(call->n_consensus, 0), SP_CYP_MAXCONS);
    uint64_t off[SP_CYP_MAXCONS + 1] = { 0 }; sp_support_summary sm[SP_CYP_MAXCONS];
    const uint64_t moff[2] = { 0, n_mappings };
    if (haps && !heads) return sp_fail(ctx, SP_ERR_INVALID_ARG, "cyp consensus support: null argument");
    sp_support_hap_head hd[SP_CYP_MAXCONS];
    const int32_t rc = sp_cyp_consensus_support_cohort_hap(ctx, 1, &reads, call, consensus, cons_cap, mappings, moff, off, cols, cols_cap, sm, ins, ins_cap, n_ins, haps, hap_cap, n_haps, haps ? hd : nullptr);
    std::memcpy(col_offset, off, sizeof(uint64_t) * ((size_t)H + 1));
    if (rc != SP_OK && !only_a_list_short(rc, ins, n_ins, ins_cap, haps, n_haps, hap_cap)) return rc;
    std::memcpy(summaries, sm, sizeof(sp_support_summary) * (size_t)H);
    if (haps && n_haps && *n_haps <= hap_cap) std::memcpy(heads, hd, sizeof(sp_support_hap_head) * (size_t)H);
    return rc;
}

int32_t sp_cyp_consensus_support_ins(sp_ctx* ctx, const sp_seqset* reads, const sp_cyp_call* call, const char* consensus, uint32_t cons_cap,
                                     const sp_cyp_read_mapping* mappings, uint64_t n_mappings, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap,
                                     sp_support_summary* summaries, sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins) {
    return sp_cyp_consensus_support_hap(ctx, reads, call, consensus, cons_cap, mappings, n_mappings, col_offset, cols, cols_cap, summaries, ins, ins_cap, n_ins, nullptr, 0, nullptr, nullptr);
}

int32_t sp_cyp_consensus_support(sp_ctx* ctx, const sp_seqset* reads, const sp_cyp_call* call, const char* consensus, uint32_t cons_cap,
                                 const sp_cyp_read_mapping* mappings, uint64_t n_mappings, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap,
                                 sp_support_summary* summaries) {
    return sp_cyp_consensus_support_ins(ctx, reads, call, consensus, cons_cap, mappings, n_mappings, col_offset, cols, cols_cap, summaries, nullptr, 0, nullptr);
}

// ---------------------------------------------------------------------------------------------------------------- cyp2d6_consensus_support.json
int32_t sp_cyp_support_json(const sp_cyp_call* call, const char* consensus, uint32_t cons_cap, const uint64_t* col_offset, const sp_pileup_col* cols,
                            const sp_support_summary* summaries, char* out, uint64_t cap, uint64_t* needed) {
    return sp_cyp_support_json_ins(call, consensus, cons_cap, col_offset, cols, summaries, nullptr, 0, nullptr, 0, nullptr, 0, out, cap, needed);
}

int32_t sp_cyp_support_json_ins(const sp_cyp_call* call, const char* consensus, uint32_t cons_cap, const uint64_t* col_offset, const sp_pileup_col* cols,
                                const sp_support_summary* summaries, const sp_pileup_ins* ins, uint64_t n_ins, const sp_cyp_read_mapping* mappings, uint64_t n_mappings,
                                const char* const* read_names, uint32_t n_read_names, char* out, uint64_t cap, uint64_t* needed) {
    return sp_cyp_support_json_hap(call, consensus, cons_cap, col_offset, cols, summaries, ins, n_ins, nullptr, 0, nullptr, 0, mappings, n_mappings, read_names, n_read_names, out, cap, needed);
}

int32_t sp_cyp_support_json_hap(const sp_cyp_call* call, const char* consensus, uint32_t cons_cap, const uint64_t* col_offset, const sp_pileup_col* cols,
                                const sp_support_summary* summaries, const sp_pileup_ins* ins, uint64_t n_ins, const sp_support_hap* haps, uint64_t n_haps,
                                const sp_support_hap_head* heads, uint64_t target0, const sp_cyp_read_mapping* mappings, uint64_t n_mappings,
                                const char* const* read_names, uint32_t n_read_names, char* out, uint64_t cap, uint64_t* needed) {
    if (!call || (cap && !out) || (n_ins && !ins) || (n_haps && (!haps || !heads))) return SP_ERR_INVALID_ARG;
    const int32_t H = call->status == 0 ? std::min<int32_t>(std::max<int32_t>(call->n_consensus, 0), SP_CYP_MAXCONS) : 0;
    if (H > 0 && (!consensus || cons_cap == 0 || !col_offset || !summaries)) return SP_ERR_INVALID_ARG;
    const SupportJsonLists L = { ins, n_ins, haps, n_haps, mappings, n_mappings, mappings ? read_names : nullptr, n_read_names };
    spj::Value root = spj::object();
    for (int32_t h = 0; h < H; ++h) {
        const sp_support_summary& sm = summaries[h];
        const char* s = consensus + (size_t)h * cons_cap;
        if (col_offset[h + 1] < col_offset[h] || col_offset[h + 1] - col_offset[h] != sm.length || strnlen(s, cons_cap) < sm.length || (sm.length && !cols)) return SP_ERR_INVALID_ARG;
        const std::string type = spi_cyp_region_label(call, h);
        root.obj.emplace_back(std::to_string(h) + "_" + type, consensus_json(sm, cols ? cols + col_offset[h] : nullptr, s, "region_type", spj::str(type), L, col_offset[h],
                                                                             n_haps ? heads + target0 + h : nullptr, target0 + (uint64_t)h));
    }
    std::string text;
    spj::write_pretty(text, root);
    return copy_out(text, out, cap, needed);
}

} // extern "C"

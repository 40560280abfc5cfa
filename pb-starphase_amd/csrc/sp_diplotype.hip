// sp_diplotype.hip -- files to files: call_diplotypes (src/diplotyper.rs:40-330) behind one handle, on top of the library's own entry points.
// Per database (sp_starphase_create): the database file, the reference FASTA, the HLA database of the hla_config genes (K1 / K2 tables), the
// CYP2D6 templates and typing tables (on a second context of the same device), every variant gene normalised.  Per sample (sp_starphase_call):
//   variant genes  VCF (+ SV VCF) -> sp_variant_gene_problem -> one sp_variant_solve_batch (K6) -> the packaging of call_diplotypes (:130-204)
//   HLA            the read loop of diplotype_hla_batch (src/hla/caller.rs:540-596) -> K1 -> buckets in QNAME order -> K8 / K2 -> new_from_mappings
//   CYP2D6         the read collection of diplotype_cyp2d6 (src/cyp2d6/caller.rs:60-139) -> K3 / K8 / K9 / K7 / K4 / K5 -> new_from_multi_mappings
// There is one pipeline, over a group of samples: sample_setup (inputs, checks) -> variant_samples / hla_group / cyp_group (one variant solve, one K1 pass
// that also names the reverse-strand reads, one HLA call and one CYP2D6 call per group; the single-sample entry points for a group of one) -> sample_result
// (the entries in one fixed order, the error precedence, the warnings).  The CYP2D6 lane runs on a host thread of its own with the second context while the
// calling thread does the variant genes and the HLA genes; every entry is built from its own lane's inputs only, so the result is the same whichever way the
// lanes ran (settings.sequential = 1 runs them one after another).
// sp_starphase_call is that pipeline for a group of one, decoding its files inside its lanes; sp_starphase_call_batch runs it per group of max_group
// samples, the host decode of the next group beside the device work of this one.
#include "sp_internal.h"
#include "sp_json.h"
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <deque>
#include <fstream>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <sys/stat.h>
#include <thread>
#include <vector>

namespace {

thread_local std::string g_create_error;        // sp_starphase_last_error(NULL): why the last create of this thread failed

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

std::string opt(const char* s) { return s ? std::string(s) : std::string(); }

// one read of a locus: QNAME and its SEQ as the file stores it (4 bits per base)
struct Read4 { std::string qname; std::vector<uint8_t> seq4; uint32_t len = 0; };

// the records of [start, end) of chrom in every BAM, in file order; a QNAME already seen (in an earlier file or region of this lane) is skipped.
// No FLAG filter: rust-htslib's records() hands out every record of the fetch (the reference filters none).  A fetch that fails counts as no reads.
int32_t collect_reads(const std::vector<std::string>& bams, const std::string& chrom, uint64_t start, uint64_t end, std::set<std::string>& seen,
                      std::vector<Read4>& out, std::string& warnings, std::string& err) {
    for (const std::string& path : bams) {
        sp_bam* bam = nullptr;
        char e[512] = {0};
        if (sp_bam_open(path.c_str(), &bam, e, sizeof e) != SP_OK) { err = "Error while opening " + path + ": " + e; return SP_ERR_INVALID_ARG; }
        const sp_bam_read* reads = nullptr; uint32_t n = 0; const char* bases = nullptr; const uint64_t* offsets = nullptr;
        if (sp_bam_fetch(bam, chrom.c_str(), start, end, 0, 0, &reads, &n, &bases, &offsets) != SP_OK) {
            warnings += "Received error \"" + opt(sp_bam_last_error(bam)) + "\" while fetching " + chrom + ":" + std::to_string(start + 1) + "-" +
                        std::to_string(end) + " in \"" + path + "\", assuming no reads for region.\n";
            sp_bam_free(bam);
            continue;
        }
        const uint8_t* seq4 = nullptr; const uint64_t* boff = nullptr; const uint32_t* lens = nullptr; uint32_t n4 = 0;
        if (sp_bam_last_seq4(bam, &seq4, &boff, &lens, &n4) != SP_OK || n4 != n) { err = "sp_bam_last_seq4 failed on " + path; sp_bam_free(bam); return SP_ERR_INVALID_ARG; }
        for (uint32_t i = 0; i < n; ++i) {
            if (!seen.insert(reads[i].qname).second) continue;
            Read4 r; r.qname = reads[i].qname; r.len = lens[i];
            r.seq4.assign(seq4 + boff[i], seq4 + boff[i + 1]);
            out.push_back(std::move(r));
        }
        sp_bam_free(bam);
    }
    return SP_OK;
}

// one SP_SEQ_BAM4 set: part after part, the reads of a part in its `order`
struct ReadPart { const std::vector<Read4>* reads; const std::vector<uint32_t>* order; };
int32_t upload_reads(sp_ctx* ctx, const std::vector<ReadPart>& parts, sp_seqset** out) {
    std::vector<uint8_t> bytes; std::vector<uint64_t> off{0}; std::vector<uint32_t> lens;
    for (const ReadPart& p : parts)
        for (uint32_t i : *p.order) { const Read4& r = (*p.reads)[i]; bytes.insert(bytes.end(), r.seq4.begin(), r.seq4.end()); off.push_back(bytes.size()); lens.push_back(r.len); }
    if (bytes.empty()) bytes.push_back(0);
    return sp_seqset_upload_format(ctx, SP_SEQ_BAM4, bytes.data(), off.data(), lens.data(), (uint32_t)lens.size(), out);
}

std::vector<uint32_t> qname_order(const std::vector<Read4>& reads) {
    std::vector<uint32_t> o(reads.size());
    for (uint32_t i = 0; i < o.size(); ++i) o[i] = i;
    std::sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) { return reads[a].qname < reads[b].qname; });    // BTreeMap<String, _> order (bytes)
    return o;
}

bool read_lines(const std::string& path, std::set<std::string>& out) {
    std::ifstream f(path);
    if (!f) return false;
    std::string line;
    while (std::getline(f, line)) { if (!line.empty() && line.back() == '\r') line.pop_back(); out.insert(line); }
    return true;
}

struct GeneDetailsPtr {
    sp_gene_details* d = nullptr;
    GeneDetailsPtr() { sp_gene_details_create(&d); }
    ~GeneDetailsPtr() { sp_gene_details_free(d); }
};

// one entry of the result, ready to be inserted: made on whichever lane computed it
struct Entry { std::string gene; std::unique_ptr<GeneDetailsPtr> details; int32_t constructor = 0; };

// the VCF records vcf_fetch reads for a gene: +-50 bp around each of its variants; fetch = selected and with variants (or an SV)
struct GeneWindow { bool fetch = false; uint64_t lo = 0, hi = 0; uint32_t n_variants = 0; };

}  // namespace

struct sp_starphase {
    sp_ctx* ctx = nullptr; bool own_ctx = false;
    sp_ctx* ctx2 = nullptr;                          // the CYP2D6 lane
    sp_database* db = nullptr;
    sp_fasta* fasta = nullptr;
    std::string err, warnings;
    sp_starphase_timing timing{};
    // settings (strings copied)
    sp_diplotype_settings s{};
    std::string include_set, exclude_set, sample_name, sv_vcf, debug_folder;
    int32_t read_debug = 0;                          // sp_starphase_set_read_debug: a debug folder also receives read_debug.json
    int32_t consensus_support = 0;                   // sp_starphase_set_consensus_support: a debug folder also receives consensus_support.json
    int32_t support_insertions = 0;                  // sp_starphase_set_support_insertions: those two files also list the inserted strings of their contested columns
    int32_t support_haplotypes = 0;                  // sp_starphase_set_support_haplotypes: those two files also list the read haplotypes at their contested columns
    int32_t cyp_vcf = 0;                             // sp_starphase_set_cyp_vcf: a debug folder also receives cyp2d6_alleles.vcf.gz, with SR / CR from the support pass
    int32_t variant_alternatives = 0;                // sp_starphase_set_variant_alternatives: a debug folder also receives variant_alternatives.json (the ten best candidates of every solved variant gene)
    int32_t cyp_alternative_reads = 0;               // sp_starphase_set_cyp_alternative_reads: a debug folder also receives cyp2d6_alternative_reads.json (those pairs read by read)
    int32_t cyp_alternatives = 0;                    // sp_starphase_set_cyp_alternatives: a debug folder also receives cyp2d6_alternatives.json (the ten best chain pairs)
    int32_t cyp_consensus_support = 0;               // sp_starphase_set_cyp_consensus_support: a debug folder also receives cyp2d6_consensus_support.json
    int32_t hla_ties = 0;                            // sp_starphase_set_hla_ties: a debug folder gets hla_ties.json, the alleles each consensus's a = 5 scan cannot tell from its winner
    int32_t hla_debug_mappings = 0;                  // sp_starphase_set_hla_debug_mappings: hla_debug.json carries the mapping of each consensus against every allowed allele
    std::set<std::string> include, exclude; bool has_include = false, has_exclude = false;
    // chromosomes the variant genes were normalised against (sp_variant_gene keeps a pointer)
    std::map<std::string, std::string> chrom_seq;
    // variant genes, in gene_entries key order
    struct VGene { std::string name, chrom, reference_allele, sv_chrom; bool has_sv = false; sp_variant_gene* g = nullptr; bool selected = true; };
    std::vector<VGene> vgenes;
    std::vector<GeneWindow> win;                     // per vgenes entry, made once by sp_starphase_create
    // HLA: the selected hla_config genes
    sp_hla_db* hla = nullptr;
    struct HGene { std::string name, chrom; uint64_t start = 0, end = 0; bool absent_capable = false; };
    std::vector<HGene> hgenes;
    std::vector<std::string> a_id, a_star;           // allele i: "HLA:HLA00001", "HLA-A*01:01:01:01" minus the gene ("01:01:01:01")
    std::vector<uint32_t> a_gene;
    // CYP2D6
    sp_cyp_db* cyp = nullptr; bool cyp_selected = false;
    std::string cyp_chrom; uint64_t cyp_start = 0, cyp_end = 0;     // extraction_region (src/cyp2d6/definitions.rs:72-99)
    std::string hla_err, cyp_err;                    // why a locus could not be set up (reported by the first call that needs it)
    // sp_starphase_call_batch: per-sample errors and warnings of the last batch, its timing
    std::vector<std::string> batch_err, batch_warn;
    sp_starphase_batch_timing batch_timing{};
    std::vector<char> hla_cons;                      // the HLA call's consensus texts (not read; kept across calls)

    bool selected(const std::string& gene) const {
        if (has_include && !include.count(gene)) return false;
        if (has_exclude && exclude.count(gene)) return false;
        return true;
    }
    int32_t fail(int32_t rc, const std::string& m) { err = m; return rc; }
};

namespace {

const char* chrom_bases(sp_starphase* h, const std::string& chrom, uint64_t* len) {
    auto it = h->chrom_seq.find(chrom);
    if (it == h->chrom_seq.end()) {
        uint32_t n = 0; const char* const* names = nullptr; const uint64_t* lengths = nullptr;
        if (sp_fasta_sequences(h->fasta, &n, &names, &lengths) != SP_OK) return nullptr;
        uint64_t L = 0; bool found = false;
        for (uint32_t i = 0; i < n; ++i) if (chrom == names[i]) { L = lengths[i]; found = true; }
        if (!found) return nullptr;
        const char* b = nullptr; uint64_t got = 0;
        if (sp_fasta_fetch(h->fasta, chrom.c_str(), 0, L, &b, &got) != SP_OK) return nullptr;
        it = h->chrom_seq.emplace(chrom, std::string(b, got)).first;
    }
    *len = it->second.size();
    return it->second.c_str();
}

// ---------------------------------------------------------------- variant genes
// A variant problem points into its sp_variant_gene, which keeps only its last problem.  This is a problem on its own: the arrays, and what the gene
// says about this problem's ids (id -> database variant or deletion, the deletion labels), so solving and packaging need the gene's static tables only.
struct OwnedProblem {
    struct Var { int32_t db_variant = -1; bool has_label = false; std::string sv_label; uint64_t sv_start = 0, sv_end = 0; };
    size_t gene = 0, entry = 0;                      // the vgenes index, the sample's entry it fills
    std::vector<uint8_t> hap_is_sv, hap_is_core, var_is_core; std::vector<int32_t> slot_off, alt_off, alt_var, obs_var, obs_gt, obs_sv_label; std::vector<int64_t> obs_ps;
    std::vector<Var> vars; std::vector<std::string> labels;
    sp_variant_problem p{};
    bool take(const sp_variant_gene* g, const sp_variant_problem& q) {
        const size_t H = (size_t)std::max(0, q.n_haps), V = (size_t)std::max(0, q.n_vars), O = (size_t)std::max(0, q.n_obs);
        slot_off.assign(q.slot_off, q.slot_off + H + 1);
        const size_t S = (size_t)slot_off[H];
        alt_off.assign(q.alt_off, q.alt_off + S + 1);
        alt_var.assign(q.alt_var, q.alt_var + alt_off[S]);
        hap_is_sv.assign(q.hap_is_sv, q.hap_is_sv + H); hap_is_core.assign(q.hap_is_core, q.hap_is_core + H);
        var_is_core.assign(q.var_is_core, q.var_is_core + V);
        obs_var.assign(q.obs_var, q.obs_var + O); obs_gt.assign(q.obs_gt, q.obs_gt + O); obs_ps.assign(q.obs_ps, q.obs_ps + O);
        obs_sv_label.assign(q.obs_sv_label, q.obs_sv_label + O);
        p = q;
        p.hap_is_sv = hap_is_sv.data(); p.hap_is_core = hap_is_core.data(); p.slot_off = slot_off.data(); p.alt_off = alt_off.data(); p.alt_var = alt_var.data();
        p.var_is_core = var_is_core.data(); p.obs_var = obs_var.data(); p.obs_gt = obs_gt.data(); p.obs_ps = obs_ps.data(); p.obs_sv_label = obs_sv_label.data();
        vars.assign(V, Var());
        for (size_t v = 0; v < V; ++v) {
            const char* label = nullptr;
            if (sp_variant_gene_problem_variant(g, (int32_t)v, &vars[v].db_variant, &label, &vars[v].sv_start, &vars[v].sv_end) != SP_OK) return false;
            vars[v].has_label = label != nullptr; vars[v].sv_label = opt(label);
        }
        labels.clear();
        for (const char* l = nullptr; sp_variant_gene_problem_sv_label(g, (int32_t)labels.size(), &l) == SP_OK;) labels.push_back(opt(l));
        return true;
    }
};

struct VarInfo { std::string name; bool is_core = true; bool is_sv = false; std::string sv_label; };

// one solved gene -> its PgxGeneDetails (call_diplotypes, src/diplotyper.rs:130-204)
int32_t package_gene(sp_starphase* h, const sp_starphase::VGene& vg, const OwnedProblem& q, const sp_variant_result& res, Entry& e) {
    const sp_variant_gene* g = vg.g;
    const sp_variant_problem& p = q.p;
    if (res.overflow) return h->fail(SP_ERR_CAPACITY, vg.name + ": more than " + std::to_string(SP_VAR_MAXDIP) + " tied diplotypes");
    // names of the problem's variants (RegionVariant labels: the database name, "structural_variant" for an SV; SVs are core variants)
    std::vector<VarInfo> var(p.n_vars);
    for (int v = 0; v < p.n_vars; ++v) {
        const OwnedProblem::Var& pv = q.vars[v];
        if (pv.db_variant >= 0) {
            uint64_t pos; const char *r, *a, *nm, *dbsnp; int64_t vid; int32_t core;
            sp_variant_gene_variant(g, (uint32_t)pv.db_variant, &pos, &r, &a, &nm, &dbsnp, &vid, &core);
            var[v] = VarInfo{opt(nm), core != 0, false, ""};
        } else var[v] = VarInfo{"structural_variant", true, true, pv.sv_label};
    }
    auto hap_name = [&](int32_t x) -> std::string {
        if (x < 0) return (size_t)(-x - 2) < q.labels.size() ? q.labels[(size_t)(-x - 2)] : std::string();
        const char* n = nullptr; const char* c = nullptr; sp_variant_gene_haplotype(g, (uint32_t)x, &n, &c); return opt(n);
    };
    auto core_name = [&](int32_t x) -> std::string {          // build_core_allele_lookup (:378-399)
        if (x < 0) { std::string l = hap_name(x); return l.substr(0, l.find('.')); }
        const char* n = nullptr; const char* c = nullptr; sp_variant_gene_haplotype(g, (uint32_t)x, &n, &c); return c ? std::string(c) : opt(n);
    };
    const bool exact_sub = res.score[0] == 0 && res.score[1] == 0 && res.score[2] == 0 && res.score[3] == 0;
    const bool exact_core = res.score[0] == 0 && res.score[1] == 0;
    sp_gene_details* d = e.details->d;
    for (int i = 0; i < res.n_dip; ++i) {
        const int32_t a = res.dip[i][0], b = res.dip[i][1];
        if (exact_sub) sp_gene_details_add_diplotype(d, hap_name(a).c_str(), hap_name(b).c_str());
        else if (exact_core) sp_gene_details_add_diplotype(d, core_name(a).c_str(), core_name(b).c_str());
        if (exact_sub || exact_core) sp_gene_details_add_simple_diplotype(d, core_name(a).c_str(), core_name(b).c_str());
        if (exact_sub) continue;
        // derive_inexact_haplotype (:1516-1550) of both sides
        std::vector<int32_t> side[2];
        spi_het_split(p, res.dip_comb[i], side[0], side[1]);
        std::string base[2]; std::vector<std::string> labels[2]; std::vector<uint8_t> vi[2]; std::vector<int32_t> st[2];
        for (int k = 0; k < 2; ++k) {
            const int32_t x = res.dip[i][k];
            if (x >= 0) {
                std::vector<int32_t> m, mi, ex;
                spi_quant_match(p, x, side[k], m, mi, ex);
                base[k] = hap_name(x);
                for (int32_t v : m)  { labels[k].push_back(var[v].name); vi[k].push_back(var[v].is_core); st[k].push_back(SP_REL_MATCH); }
                for (int32_t v : mi) { labels[k].push_back(var[v].name); vi[k].push_back(var[v].is_core); st[k].push_back(SP_REL_MISSING); }
                for (int32_t v : ex) { labels[k].push_back(var[v].name); vi[k].push_back(var[v].is_core); st[k].push_back(SP_REL_UNEXPECTED); }
            } else {                     // the SV short-circuit (:1414-1431): the first label names the haplotype, the others are unexpected core variants
                bool first = true;
                for (int32_t v : side[k]) {
                    if (!var[v].is_sv) continue;
                    if (first) { base[k] = var[v].sv_label; first = false; continue; }
                    labels[k].push_back(var[v].sv_label); vi[k].push_back(1); st[k].push_back(SP_REL_UNEXPECTED);
                }
                if (first) base[k] = hap_name(x);
            }
        }
        std::vector<const char*> l0, l1;
        for (auto& s : labels[0]) l0.push_back(s.c_str());
        for (auto& s : labels[1]) l1.push_back(s.c_str());
        sp_gene_details_add_inexact_diplotype(d, base[0].c_str(), (uint32_t)l0.size(), l0.data(), vi[0].data(), st[0].data(),
                                              base[1].c_str(), (uint32_t)l1.size(), l1.data(), vi[1].data(), st[1].data());
    }
    // variant_details: the observed variants in NormalizedVariant order
    for (int o = 0; o < p.n_obs; ++o) {
        const OwnedProblem::Var& pv = q.vars[(size_t)p.obs_var[o]];
        const uint64_t s0 = pv.sv_start, s1 = pv.sv_end;
        sp_variant_detail det{};
        det.genotype = p.obs_gt[o]; det.phase_set = p.obs_ps[o];
        if (pv.db_variant >= 0) {
            uint64_t pos; const char *r, *a, *nm, *dbsnp; int64_t vid; int32_t core;
            sp_variant_gene_variant(g, (uint32_t)pv.db_variant, &pos, &r, &a, &nm, &dbsnp, &vid, &core);
            det.variant_id = (uint64_t)vid; det.variant_name = nm; det.dbsnp = dbsnp; det.chrom = vg.chrom.c_str(); det.position = pos;
            det.reference = r; det.alternate = a; det.is_core_variant = core;
        } else {
            det.variant_id = UINT64_MAX; det.variant_name = "structural_variant"; det.dbsnp = nullptr; det.chrom = vg.sv_chrom.c_str(); det.position = s0;
            det.reference = ""; det.alternate = ""; det.sv_label = pv.has_label ? pv.sv_label.c_str() : nullptr; det.sv_start = s0; det.sv_end = s1; det.is_core_variant = 1;
        }
        if (sp_gene_details_add_variant(d, &det) != SP_OK) return h->fail(SP_ERR_INVALID_ARG, vg.name + ": bad variant detail");
    }
    e.constructor = exact_sub ? SP_DETAILS_SUBALLELE_MATCH : exact_core ? SP_DETAILS_CORE_MATCH : SP_DETAILS_INEXACT_DIPLOTYPES;
    return SP_OK;
}

// the VCF (+ SV VCF) records of every selected gene with variants (+-50 bp around each variant), read by the decode.  fail_at: the vgenes index of the
// first gene whose fetch failed (0 with fail_rc set: the files themselves); the genes before it still build their problems first.
struct VcfGene { std::vector<uint64_t> pos; std::vector<std::string> ref, alt; std::vector<int32_t> gt; std::vector<int64_t> ps; std::vector<sp_vcf_deletion> dels; };
struct VcfFetch { std::vector<VcfGene> genes; size_t fail_at = SIZE_MAX; int32_t fail_rc = SP_OK; std::string fail_err; };

void vcf_fetch(sp_starphase* h, const std::vector<GeneWindow>& win, const std::string& vcf_path, const std::string& sv_path, const std::string& sample_in, VcfFetch& F) {
    F.genes.assign(h->vgenes.size(), VcfGene());
    auto fail = [&](size_t at, const std::string& m) { F.fail_at = at; F.fail_rc = SP_ERR_INVALID_ARG; F.fail_err = m; };
    sp_vcf* vcf = nullptr; sp_vcf* sv = nullptr;
    char e[512] = {0};
    if (sp_vcf_open(vcf_path.c_str(), &vcf, e, sizeof e) != SP_OK) return fail(0, "Error while opening " + vcf_path + ": " + e);
    std::unique_ptr<sp_vcf, void (*)(sp_vcf*)> vcf_guard(vcf, sp_vcf_free);
    std::string sample = sample_in;
    if (sample.empty()) {
        uint32_t n = 0; const char* const* names = nullptr;
        if (sp_vcf_samples(vcf, &n, &names) != SP_OK || n == 0) return fail(0, "No samples found in VCF: " + vcf_path);
        sample = names[0];
    }
    std::unique_ptr<sp_vcf, void (*)(sp_vcf*)> sv_guard(nullptr, sp_vcf_free);
    if (!sv_path.empty()) {
        if (sp_vcf_open(sv_path.c_str(), &sv, e, sizeof e) != SP_OK) return fail(0, "Error while opening " + sv_path + ": " + e);
        sv_guard.reset(sv);
    }
    for (size_t i = 0; i < h->vgenes.size(); ++i) {
        const sp_starphase::VGene& vg = h->vgenes[i];
        if (!win[i].fetch) continue;
        VcfGene& G = F.genes[i];
        const sp_vcf_allele* alleles = nullptr; uint32_t n_alleles = 0;
        if (win[i].n_variants && sp_vcf_alleles(vcf, sample.c_str(), vg.chrom.c_str(), win[i].lo, win[i].hi, &alleles, &n_alleles) != SP_OK)
            return fail(i, vg.name + ": " + opt(sp_vcf_last_error(vcf)));
        for (uint32_t a = 0; a < n_alleles; ++a) {
            G.pos.push_back(alleles[a].position); G.ref.push_back(opt(alleles[a].ref)); G.alt.push_back(opt(alleles[a].alt));
            G.gt.push_back(alleles[a].gt); G.ps.push_back(alleles[a].ps);
        }
        const sp_vcf_deletion* dels = nullptr; uint32_t n_dels = 0;
        if (sv && vg.has_sv && sp_vcf_deletions(sv, sample.c_str(), vg.sv_chrom.c_str(), 0, UINT64_MAX >> 2, &dels, &n_dels) != SP_OK)
            return fail(i, vg.name + ": " + opt(sp_vcf_last_error(sv)));
        G.dels.assign(dels, dels + n_dels);
    }
}

int32_t vcf_problem(sp_starphase* h, size_t i, const VcfGene& G, sp_variant_problem& p) {
    std::vector<sp_vcf_allele> al(G.pos.size());
    for (size_t a = 0; a < al.size(); ++a) { al[a] = sp_vcf_allele{}; al[a].position = G.pos[a]; al[a].ref = G.ref[a].c_str(); al[a].alt = G.alt[a].c_str(); al[a].gt = G.gt[a]; al[a].ps = G.ps[a]; }
    sp_starphase::VGene& vg = h->vgenes[i];
    p = sp_variant_problem{};
    if (sp_variant_gene_problem(vg.g, (uint32_t)al.size(), al.data(), (uint32_t)G.dels.size(), G.dels.data(), h->s.max_sv_length, &p) != SP_OK)
        return h->fail(SP_ERR_INVALID_ARG, vg.name + ": " + opt(sp_variant_gene_last_error(vg.g)));
    return SP_OK;
}

// one sample's variant genes
struct VarSample {
    bool has_vcf = false; std::string vcf, sv, sample;
    VcfFetch vf;                                     // read by vcf_fetch
    int32_t rc = SP_OK; std::string err;
    std::vector<Entry> entries; std::vector<OwnedProblem> probs; size_t res0 = 0;
    std::string alt_folder;                          // sp_starphase_set_variant_alternatives: where variant_alternatives.json goes (empty: not asked for)
};

// variant_alternatives.json of the samples that ask for it: ONE sp_variant_alternatives_batch over their problems, then one object per sample, keyed by gene name
// in name order (the order of vgenes), each value sp_variant_alternatives_json's text with the names package_gene uses
void variant_alternatives_save(sp_starphase* h, const std::vector<VarSample*>& solving) {
    std::vector<const sp_variant_problem*> pp; std::vector<VarSample*> want;
    for (VarSample* b : solving) if (b->rc == SP_OK && !b->alt_folder.empty()) { want.push_back(b); for (auto& q : b->probs) pp.push_back(&q.p); }
    if (want.empty()) return;
    const uint32_t N = SP_VAR_ALTERNATIVES;
    std::vector<sp_variant_alt> alts(std::max<size_t>(1, pp.size() * N)); std::vector<sp_variant_alt_info> infos(std::max<size_t>(1, pp.size()));
    if (!pp.empty()) {
        const int32_t rc = sp_variant_alternatives_batch(h->ctx, (uint32_t)pp.size(), pp.data(), N, alts.data(), infos.data(), nullptr);
        if (rc != SP_OK) { for (VarSample* b : want) { b->rc = rc; b->err = "sp_variant_alternatives_batch: " + opt(sp_last_error(h->ctx)); } return; }
    }
    size_t first = 0;
    for (VarSample* b : want) {
        std::string text = "{";
        const size_t base = first; first += b->probs.size();
        for (size_t k = 0; k < b->probs.size(); ++k) {
            const size_t at = base + k;
            const OwnedProblem& q = b->probs[k];
            const sp_starphase::VGene& vg = h->vgenes[q.gene];
            std::vector<std::string> hap((size_t)std::max(0, q.p.n_haps)), hap_core(hap.size()), var((size_t)std::max(0, q.p.n_vars));
            for (size_t x = 0; x < hap.size(); ++x) {
                const char* n = nullptr; const char* c = nullptr; sp_variant_gene_haplotype(vg.g, (uint32_t)x, &n, &c);
                hap[x] = opt(n); hap_core[x] = c ? std::string(c) : opt(n);
            }
            for (size_t v = 0; v < var.size(); ++v) {
                var[v] = "structural_variant";
                if (q.vars[v].db_variant >= 0) {
                    uint64_t pos; const char *r, *a, *nm, *dbsnp; int64_t vid; int32_t core;
                    sp_variant_gene_variant(vg.g, (uint32_t)q.vars[v].db_variant, &pos, &r, &a, &nm, &dbsnp, &vid, &core);
                    var[v] = opt(nm);
                }
            }
            std::vector<const char*> hp, hcp, vp, lp;
            for (auto& x : hap) hp.push_back(x.c_str());
            for (auto& x : hap_core) hcp.push_back(x.c_str());
            for (auto& x : var) vp.push_back(x.c_str());
            for (auto& x : q.labels) lp.push_back(x.c_str());
            uint64_t need = 0;
            int32_t rc = sp_variant_alternatives_json(&q.p, &infos[at], alts.data() + at * N, hp.data(), hcp.data(), lp.data(), (uint32_t)lp.size(), vp.data(), nullptr, 0, &need);
            std::string entry((size_t)need, '\0');
            if (rc == SP_OK) rc = sp_variant_alternatives_json(&q.p, &infos[at], alts.data() + at * N, hp.data(), hcp.data(), lp.data(), (uint32_t)lp.size(), vp.data(), &entry[0], need, &need);
            if (rc != SP_OK) { b->rc = rc; b->err = vg.name + ": bad variant alternatives"; break; }
            entry.resize(std::strlen(entry.c_str()));
            std::string nested;
            for (char ch : entry) { nested += ch; if (ch == '\n') nested += "  "; }
            std::string key;
            spj::write_string(key, vg.name);
            text += std::string(k ? ",\n  " : "\n  ") + key + ": " + nested;
        }
        text += b->probs.empty() ? "}" : "\n}";
        if (b->rc == SP_OK) {
            const std::string path = b->alt_folder + "/variant_alternatives.json";
            FILE* f = std::fopen(path.c_str(), "wb");
            if (!f || std::fwrite(text.data(), 1, text.size(), f) != text.size()) { if (f) std::fclose(f); b->rc = SP_ERR_INVALID_ARG; b->err = "Error while writing " + path; continue; }
            std::fclose(f);
        }
    }
}

// call_diplotypes' gene loop (src/diplotyper.rs:94-204) for every sample of `group` whose VCF was read: each sample's problems, ONE
// sp_variant_solve_batch over all of them, then the entries sample by sample.  A failure and its text belong to the sample that has it: when the
// shared launch fails, each sample's problems are solved once more on their own.
void variant_samples(sp_starphase* h, const std::vector<VarSample*>& group) {
    std::vector<const sp_variant_problem*> pp;
    for (VarSample* b : group) {
        if (!b->has_vcf || b->rc != SP_OK) continue;
        for (size_t i = 0; i < h->vgenes.size() && b->rc == SP_OK; ++i) {
            if (i >= b->vf.fail_at) { b->rc = b->vf.fail_rc; b->err = b->vf.fail_err; break; }
            sp_starphase::VGene& vg = h->vgenes[i];
            if (!vg.selected) continue;
            Entry en; en.gene = vg.name; en.details.reset(new GeneDetailsPtr());
            if (!h->win[i].fetch) {                     // "No variants found ..., returning default reference allele." (:94-105)
                sp_gene_details_add_diplotype(en.details->d, vg.reference_allele.c_str(), vg.reference_allele.c_str());
                sp_gene_details_add_simple_diplotype(en.details->d, vg.reference_allele.c_str(), vg.reference_allele.c_str());
                en.constructor = SP_DETAILS_SUBALLELE_MATCH;
                b->entries.push_back(std::move(en));
                continue;
            }
            sp_variant_problem p{};
            const int32_t rc = vcf_problem(h, i, b->vf.genes[i], p);
            if (rc != SP_OK) { b->rc = rc; b->err = h->err; break; }
            b->probs.emplace_back();
            OwnedProblem& q = b->probs.back(); q.gene = i; q.entry = b->entries.size();
            if (!q.take(vg.g, p)) { b->rc = SP_ERR_INVALID_ARG; b->err = vg.name + ": bad problem variant"; break; }
            b->entries.push_back(std::move(en));
        }
    }
    std::vector<VarSample*> solving;
    for (VarSample* b : group) if (b->has_vcf && b->rc == SP_OK) { b->res0 = pp.size(); for (auto& q : b->probs) pp.push_back(&q.p); solving.push_back(b); }
    std::vector<sp_variant_result> res(pp.size());
    if (!pp.empty()) {
        std::vector<int32_t> rcs(pp.size(), SP_OK);
        const int32_t rc = sp_variant_solve_batch(h->ctx, (uint32_t)pp.size(), pp.data(), res.data(), rcs.data());
        if (rc != SP_OK && solving.size() == 1) { solving[0]->rc = rc; solving[0]->err = "sp_variant_solve_batch: " + opt(sp_last_error(h->ctx)); }
        else if (rc != SP_OK) {
            for (VarSample* b : solving) {
                const size_t n = b->probs.size();
                if (n == 0) continue;
                std::vector<int32_t> own(n, SP_OK);
                const int32_t rb = sp_variant_solve_batch(h->ctx, (uint32_t)n, pp.data() + b->res0, res.data() + b->res0, own.data());
                if (rb != SP_OK) { b->rc = rb; b->err = "sp_variant_solve_batch: " + opt(sp_last_error(h->ctx)); }
            }
        }
    }
    variant_alternatives_save(h, solving);
    for (VarSample* b : solving) {
        for (size_t k = 0; k < b->probs.size() && b->rc == SP_OK; ++k) {
            const OwnedProblem& q = b->probs[k];
            const int32_t rc = package_gene(h, h->vgenes[q.gene], q, res[b->res0 + k], b->entries[q.entry]);
            if (rc != SP_OK) { b->rc = rc; b->err = h->err; }
        }
        b->probs.clear();
    }
}

// ---------------------------------------------------------------- HLA
// the read loop (src/hla/caller.rs:540-596): genes in hla_config order, every BAM in the given order, a QNAME once; searched[r] = the gene whose
// region handed out read r
int32_t hla_collect(sp_starphase* h, const std::vector<std::string>& bams, std::vector<Read4>& reads, std::vector<uint32_t>& searched, std::string& warnings,
                    std::string& err) {
    std::set<std::string> seen;
    for (size_t g = 0; g < h->hgenes.size(); ++g) {
        if (collect_reads(bams, h->hgenes[g].chrom, h->hgenes[g].start, h->hgenes[g].end, seen, reads, warnings, err) != SP_OK) return SP_ERR_INVALID_ARG;
        searched.resize(reads.size(), (uint32_t)g);
    }
    return SP_OK;
}

// the call configuration of every gene of one sample, from the sample's records (NORMALIZING_HLA_GENES, src/hla/alleles.rs:49-59)
void hla_configs(sp_starphase* h, const sp_hla_realign* rec, uint32_t n, sp_hla_call_config* cfg) {
    const size_t G = h->hgenes.size();
    std::vector<uint32_t> norm;
    for (size_t g = 0; g < G; ++g) if (h->hgenes[g].name == "HLA-DRB1") norm.push_back((uint32_t)g);
    double coverage = -1.0;
    sp_hla_normalized_coverage(rec, n, norm.data(), (uint32_t)norm.size(), &coverage);
    for (size_t g = 0; g < G; ++g) {
        sp_hla_call_config& c = cfg[g];
        c = sp_hla_call_config{};
        c.min_consensus_count = (int32_t)h->s.min_consensus_count; c.dual_max_ed_delta = (int32_t)h->s.dual_max_ed_delta;
        c.min_consensus_fraction = h->s.min_consensus_fraction; c.expected_maf = h->s.expected_maf; c.min_cdf = h->s.min_cdf_prob;
        c.require_dna = h->s.hla_require_dna; c.disable_cdna = h->s.disable_cdna_scoring; c.absent_capable = h->hgenes[g].absent_capable;
        c.normalized_coverage = coverage;
    }
}

// read_debug.json (sp_starphase_set_read_debug): the reference's `read_debug` (src/hla/caller.rs:536,575-577,631-635) -- an HlaDebug whose read_mapping_stats hold, per
// gene and QNAME, the ReadMappingStats realign_record made for a read it realigned (src/hla/realigner.rs:198-201): the accepted allele as best match and the one DNA
// mapping against it with minimap2's CIGAR and MD; no dual statistics.  Included are the reads with is_realigned() -- a RealignedHlaRecord exists --, in the bucket of
// the accepted allele's gene: the records with status 0.  A status-3 record (the segment did not map forward to the gene reference, realigner.rs:332-342) has
// realigned_record None in the reference: its PgxMappingDetails are kept but it gets no read_debug entry, like status 1 and 2.  best_match_star is the star string of
// the read's PgxMappingDetails ("HLA-A*01:01:01:01"), as this library's hla_debug.json writes it for the consensuses.
// The CIGARs come from sp_hla_realign_cigars on the set the K1 pass ran on (positions of the set; a row too short for a read's ops is run again with room).
struct ReadCigars { std::vector<uint32_t> cigar, n; uint32_t stride = 0; };
int32_t read_cigars(sp_starphase* h, const sp_seqset* set, const sp_hla_realign* rec, uint32_t R, ReadCigars* out, std::string& err) {
    out->stride = 256; out->n.assign(R, 0);
    for (int attempt = 0; attempt < 2; ++attempt) {
        out->cigar.assign((size_t)R * out->stride, 0);
        const int32_t rc = sp_hla_realign_cigars(h->ctx, h->hla, set, rec, R, out->cigar.data(), out->stride, out->n.data());
        if (rc != SP_OK) { err = "sp_hla_realign_cigars: " + opt(sp_last_error(h->ctx)); return rc; }
        uint32_t most = 0;
        for (uint32_t x : out->n) most = std::max(most, x);
        if (most <= out->stride) break;
        out->stride = most;
    }
    return SP_OK;
}
int32_t read_debug_save(sp_starphase* h, const std::vector<Read4>& reads, const std::vector<uint32_t>& pos_of, const sp_hla_realign* rec, const ReadCigars& cg,
                        uint32_t cg_first, const std::string& debug_folder, std::string& err) {
    sp_hla_debug* dbg = nullptr;
    sp_hla_debug_create(&dbg);
    std::unique_ptr<sp_hla_debug, void (*)(sp_hla_debug*)> guard(dbg, sp_hla_debug_free);
    std::map<int32_t, std::string> target;                           // the accepted alleles in hg38 orientation
    std::vector<char> cs, md;
    for (uint32_t r = 0; r < reads.size(); ++r) {
        const sp_hla_realign& q = rec[pos_of[r]];
        if (q.status != 0 || q.best_allele < 0) continue;
        const uint32_t a = (uint32_t)q.best_allele;
        auto t = target.find(q.best_allele);
        if (t == target.end()) t = target.emplace(q.best_allele, spi_hla_allele_fwd(h->ctx, h->hla, a)).first;
        const size_t at = (size_t)cg_first + pos_of[r];
        const sp_affine_aln aln = { q.mm2_score, q.mm2_nm, q.mm2_q_start, q.mm2_q_end, q.mm2_t_start, q.mm2_t_end };
        const size_t cap = 12 * ((size_t)cg.n[at] + 2) + (size_t)std::max(0, q.mm2_t_end - q.mm2_t_start) + 32;
        cs.resize(cap); md.resize(cap);
        uint64_t match_len = 0;
        int32_t rc = sp_affine_cigar_strings(&aln, cg.cigar.data() + at * cg.stride, cg.n[at], t->second.data(), t->second.size(), cs.data(), (uint32_t)cap, md.data(), (uint32_t)cap, &match_len);
        if (rc != SP_OK) { err = "read_debug.json: the CIGAR of " + reads[r].qname + " does not spell its mapping"; return rc; }
        sp_detailed_mapping dm{}; dm.present = 1;
        dm.query_len = reads[r].len; dm.target_len = t->second.size(); dm.match_len = match_len; dm.nm = (uint64_t)q.mm2_nm;
        dm.query_unmapped = reads[r].len - (uint64_t)(q.mm2_q_end - q.mm2_q_start); dm.target_unmapped = t->second.size() - (uint64_t)(q.mm2_t_end - q.mm2_t_start);
        dm.cigar = cs.data(); dm.md = md.data();
        const std::string& gene = h->hgenes[h->a_gene[a]].name; const std::string star = gene + "*" + h->a_star[a];
        rc = sp_hla_debug_add_read(dbg, gene.c_str(), reads[r].qname.c_str(), h->a_id[a].c_str(), star.c_str());
        if (rc == SP_OK) rc = sp_hla_debug_add_mapping(dbg, gene.c_str(), reads[r].qname.c_str(), h->a_id[a].c_str(), nullptr, &dm);
        if (rc != SP_OK) { err = std::string("read_debug.json: ") + sp_hla_debug_last_error(dbg); return rc; }
    }
    const std::string path = debug_folder + "/read_debug.json";
    if (sp_hla_debug_save(dbg, path.c_str()) != SP_OK) { err = "Error while writing " + path; return SP_ERR_INVALID_ARG; }
    return SP_OK;
}

// the per-allele mappings of a group's consensuses (sp_starphase_set_hla_debug_mappings): ONE batched map over every consensus of the group's samples that have a debug
// folder; item[(gene * 2 + k)] of a sample = its item in the map, -1: no consensus, or one that does not place
struct HlaMaps { sp_hla_map* map = nullptr; ~HlaMaps() { sp_hla_map_free(map); } };

// ReadMappingStats::add_mapping for every allowed allele of one consensus (score_read with all_hla_targets, src/hla/caller.rs:1398,1473-1476): keyed by the star allele,
// cdna_mapping / dna_mapping from the map (DetailedMappingStats::from_mapping, src/hla/debug.rs:161-182: query = allele, target = consensus).  A star allele met twice is
// the reference's "Entry ... is already occupied!" error; here the first entry stays and the later one is skipped with a warning.
int32_t hla_debug_mappings_add(sp_starphase* h, sp_hla_debug* dbg, const std::string& gene, const std::string& who, const sp_hla_map* map, uint32_t item, std::string& warnings, std::string& err) {
    uint32_t n = 0; const uint32_t* alleles = nullptr; const int32_t* st = nullptr;
    int32_t rc = sp_hla_map_item(map, item, nullptr, &n, &alleles, nullptr, nullptr, &st);
    if (rc != SP_OK) { err = "hla_debug.json: " + opt(sp_hla_map_last_error(map)); return rc; }
    const char* seq[2] = { nullptr, nullptr }; uint32_t len[2] = { 0, 0 };
    for (int L = 0; L < 2; ++L) sp_hla_map_consensus_seq(map, item, L, &seq[L], &len[L]);
    const std::string target[2] = { std::string(seq[0] ? seq[0] : "", len[0]), std::string(seq[1] ? seq[1] : "", len[1]) };
    std::set<std::string> seen;
    std::string cs, md;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t a = alleles[k];
        const std::string& key = h->a_star[a];
        if (!seen.insert(key).second) {
            warnings += "hla_debug.json: " + gene + " " + who + ": star allele " + key + " of " + h->a_id[a] + " is already in the mapping_stats; entry skipped\n";
            continue;
        }
        sp_detailed_mapping dm[2]; std::string strings[2][2]; bool have[2] = { false, false };
        for (int L = 0; L < 2; ++L) {
            sp_affine_aln aln; uint32_t nc = 0; const uint32_t* ops = nullptr;
            rc = sp_hla_map_mapping(map, item, k, L, &aln, nullptr, &nc, &ops);
            if (rc != SP_OK) { err = "hla_debug.json: " + opt(sp_hla_map_last_error(map)); return rc; }
            if (aln.score <= 0 || (L == 0 && h->s.disable_cdna_scoring)) continue;
            const size_t cap = 12 * ((size_t)nc + 2) + (size_t)(aln.b_end - aln.b_start) + 32;
            cs.assign(cap, 0); md.assign(cap, 0);
            uint64_t match_len = 0;
            rc = sp_affine_cigar_strings_eqx(&aln, ops, nc, target[L].data(), target[L].size(), cs.data(), (uint32_t)cap, md.data(), (uint32_t)cap, &match_len);
            if (rc != SP_OK) { err = "hla_debug.json: the CIGAR of " + h->a_id[a] + " does not spell its mapping"; return rc; }
            strings[L][0] = cs.c_str(); strings[L][1] = md.c_str();
            const int32_t qlen = st[(size_t)k * 6 + 3 * L];                      // the allele's length at this level (stats_mm2)
            sp_detailed_mapping& d = dm[L]; d = sp_detailed_mapping{};
            d.present = 1; d.query_len = (uint64_t)qlen; d.target_len = target[L].size(); d.match_len = match_len; d.nm = (uint64_t)aln.nm;
            d.query_unmapped = (uint64_t)(qlen - (aln.a_end - aln.a_start)); d.target_unmapped = (uint64_t)(target[L].size() - (size_t)(aln.b_end - aln.b_start));
            d.cigar = strings[L][0].c_str(); d.md = strings[L][1].c_str();
            have[L] = true;
        }
        rc = sp_hla_debug_add_mapping(dbg, gene.c_str(), who.c_str(), key.c_str(), have[0] ? &dm[0] : nullptr, have[1] ? &dm[1] : nullptr);
        if (rc != SP_OK) { err = std::string("hla_debug.json: ") + sp_hla_debug_last_error(dbg); return rc; }
    }
    return SP_OK;
}

// consensus_support.json of one sample (sp_starphase_set_consensus_support): the tables of the group's one support pass that belong to this sample.  off / sm are
// indexed by gene * 2 + consensus; cons holds the sample's hg38-forward consensuses, cap bytes each.  A sample without reads has no view and writes an empty object.
struct SupportView { const uint64_t* off; const sp_pileup_col* cols; const sp_support_summary* sm; const char* cons; uint32_t cap; const sp_pileup_ins* ins; uint64_t n_ins;
                     const sp_support_hap* haps = nullptr; uint64_t n_haps = 0; const sp_support_hap_head* heads = nullptr; uint64_t n_heads = 0, slot0 = 0; };   // slot0: the sample's first slot in the group's pass
// the lists of a support pass (sp_starphase_set_support_insertions / _haplotypes): each stays empty when it is not asked for
struct SupportLists { std::vector<sp_pileup_ins> ins; std::vector<sp_support_hap> haps; std::vector<sp_support_hap_head> heads; };
// a support call with the lists that are asked for: `call(ins, ins_cap, &n_ins, haps, hap_cap, &n_haps, heads)`, the arguments of a list that is not asked for NULL.
// Without a list it is called once; with one, with room for a guess (16,384 records: 0.9 MB of insertions; a list that is longer costs the pass another run) and
// again with the room it asked for -- each list can ask once, the insertion list alone is asked once
template <class F> int32_t support_with_lists(SupportLists& L, bool want_ins, bool want_haps, size_t n_heads, F call) {
    if (want_ins && L.ins.size() < 16384) L.ins.resize(16384);
    if (want_haps && L.haps.size() < 16384) L.haps.resize(16384);
    if (want_haps) L.heads.assign(std::max<size_t>(n_heads, 1), sp_support_hap_head{});
    uint64_t n_i = 0, n_h = 0;
    int32_t rc = SP_OK;
    for (int attempt = 0, calls = want_haps ? 3 : want_ins ? 2 : 1; attempt < calls; ++attempt) {
        rc = call(want_ins ? L.ins.data() : nullptr, (uint64_t)(want_ins ? L.ins.size() : 0), want_ins ? &n_i : nullptr,
                  want_haps ? L.haps.data() : nullptr, (uint64_t)(want_haps ? L.haps.size() : 0), want_haps ? &n_h : nullptr, want_haps ? L.heads.data() : nullptr);
        if (rc != SP_ERR_CAPACITY) break;
        bool grew = false;
        if (want_ins && n_i > L.ins.size()) { L.ins.resize((size_t)n_i); grew = true; }
        if (want_haps && n_h > L.haps.size()) { L.haps.resize((size_t)n_h); grew = true; }
        if (!grew) break;
    }
    L.ins.resize(rc == SP_OK && want_ins ? (size_t)n_i : 0); L.haps.resize(rc == SP_OK && want_haps ? (size_t)n_h : 0);
    return rc;
}
int32_t consensus_support_save(sp_starphase* h, const sp_hla_call* calls, const SupportView* view, const std::string& debug_folder, std::string& err) {
    const size_t G = h->hgenes.size();
    std::vector<sp_support_entry> entries; std::vector<std::string> keep; keep.reserve(G * 4);
    std::vector<uint64_t> col_base;                                  // of each entry's two consensuses, in the support pass's column space (the list's)
    std::vector<uint64_t> hap_target;                                // ... and their slots in the pass (the haplotype list's targets)
    for (size_t g = 0; view && g < G; ++g) {
        if (calls[g].status == 1) continue;
        sp_support_entry en; std::memset(&en, 0, sizeof en);
        en.gene = h->hgenes[g].name.c_str();
        for (int k = 0; k < 2; ++k) {
            if (k == 1 && !calls[g].is_dual) continue;
            const uint64_t lo = view->off[g * 2 + k], hi = view->off[g * 2 + k + 1];
            if (hi == lo) continue;
            const char* fwd = view->cons + (g * 2 + k) * (size_t)view->cap;
            std::string strand(fwd, (size_t)(hi - lo));
            if (!spi_hla_gene_fwd(h->hla, (uint32_t)g)) {
                std::reverse(strand.begin(), strand.end());
                for (char& c : strand) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
            }
            keep.push_back(std::move(strand)); en.consensus[k] = keep.back().c_str();
            const int32_t t = k ? calls[g].typed2 : calls[g].typed1;
            if (t >= 0) { keep.push_back(h->hgenes[h->a_gene[t]].name + "*" + h->a_star[t]); en.typed_allele[k] = keep.back().c_str(); }
            en.cols[k] = view->cols + lo; en.summary[k] = view->sm + g * 2 + k;
        }
        entries.push_back(en);
        col_base.push_back(view->off[g * 2]); col_base.push_back(view->off[g * 2 + 1]);
        hap_target.push_back(view->slot0 + g * 2); hap_target.push_back(view->slot0 + g * 2 + 1);
    }
    // (the list is the whole group's: a sample none of whose genes has a call has no entry, no column of the list is its own, and its file is the empty object)
    const bool listed = view && view->ins && !entries.empty();
    const sp_pileup_ins* ins = listed ? view->ins : nullptr; const uint64_t n_ins = listed ? view->n_ins : 0;
    const bool hap_listed = view && view->haps && view->n_haps && !entries.empty();
    const sp_support_hap* haps = hap_listed ? view->haps : nullptr; const uint64_t n_haps = hap_listed ? view->n_haps : 0;
    const sp_support_hap_head* heads = hap_listed ? view->heads : nullptr; const uint64_t n_heads = hap_listed ? view->n_heads : 0;
    uint64_t need = 0;
    int32_t rc = sp_consensus_support_json_hap(entries.data(), (uint32_t)entries.size(), col_base.data(), ins, n_ins, haps, n_haps, heads, n_heads, hap_target.data(), nullptr, 0, nullptr, 0, &need);
    if (rc != SP_OK && rc != SP_ERR_CAPACITY) { err = "consensus_support.json: the tables do not fit their consensuses"; return rc; }
    std::string text((size_t)need, '\0');
    rc = sp_consensus_support_json_hap(entries.data(), (uint32_t)entries.size(), col_base.data(), ins, n_ins, haps, n_haps, heads, n_heads, hap_target.data(), nullptr, 0, &text[0], need, &need);
    if (rc != SP_OK) { err = "consensus_support.json: the tables do not fit their consensuses"; return rc; }
    const std::string path = debug_folder + "/consensus_support.json";
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(text.data(), 1, (size_t)need - 1, f) != (size_t)need - 1) { if (f) std::fclose(f); err = "Error while writing " + path; return SP_ERR_INVALID_ARG; }
    std::fclose(f);
    return SP_OK;
}

// hla_ties.json of one sample (sp_starphase_set_hla_ties): the a = 5 scan's classes of the group's one map that belong to this sample's consensuses.  map_item is
// indexed by gene * 2 + consensus (-1: the consensus has no item).  A sample without reads has no map and writes an empty object.
int32_t hla_ties_save(sp_starphase* h, const sp_hla_call* calls, const sp_hla_map* maps, const int32_t* map_item, const std::string& debug_folder, std::string& err) {
    const size_t G = h->hgenes.size();
    auto star = [&](uint32_t a) { return h->hgenes[h->a_gene[a]].name + "*" + h->a_star[a]; };
    std::vector<sp_hla_ties_entry> entries;
    std::deque<std::string> keep; std::deque<std::vector<const char*>> names; std::deque<std::array<uint32_t, 5>> counts;     // (deques: what the entries point to stays where it is)
    for (size_t g = 0; maps && map_item && g < G; ++g) {
        if (calls[g].status == 1) continue;
        sp_hla_ties_entry en; std::memset(&en, 0, sizeof en);
        en.gene = h->hgenes[g].name.c_str();
        for (int k = 0; k < 2; ++k) {
            if ((k == 1 && !calls[g].is_dual) || map_item[g * 2 + k] < 0) continue;
            const uint32_t item = (uint32_t)map_item[g * 2 + k];
            uint32_t n = 0; const uint32_t* alleles = nullptr; int32_t best_mm2 = -1; const uint8_t* cls = nullptr;
            counts.emplace_back();
            int32_t rc = sp_hla_map_item(maps, item, nullptr, &n, &alleles, nullptr, &best_mm2, nullptr);
            if (rc == SP_OK) rc = sp_hla_map_ties(maps, item, 1, &cls, counts.back().data());
            if (rc != SP_OK) { err = "hla_ties.json: " + opt(sp_hla_map_last_error(maps)); return rc; }
            names.emplace_back();
            for (uint32_t x = 0; x < n; ++x) { keep.push_back(star(alleles[x])); names.back().push_back(keep.back().c_str()); }
            en.present[k] = 1; en.scan[k] = 1; en.n_alleles[k] = n; en.cls[k] = cls; en.counts[k] = counts.back().data(); en.names[k] = names.back().data();
            const int32_t t = k ? calls[g].typed2 : calls[g].typed1;
            if (t >= 0) { keep.push_back(star((uint32_t)t)); en.typed_allele[k] = keep.back().c_str(); }
            if (best_mm2 >= 0) { keep.push_back(star((uint32_t)best_mm2)); en.winner[k] = keep.back().c_str(); }
        }
        entries.push_back(en);
    }
    uint64_t need = 0;
    int32_t rc = sp_hla_ties_json(entries.data(), (uint32_t)entries.size(), nullptr, 0, &need);
    if (rc != SP_OK && rc != SP_ERR_CAPACITY) { err = "hla_ties.json: the classes do not fit their alleles"; return rc; }
    std::string text((size_t)need, '\0');
    rc = sp_hla_ties_json(entries.data(), (uint32_t)entries.size(), &text[0], need, &need);
    if (rc != SP_OK) { err = "hla_ties.json: the classes do not fit their alleles"; return rc; }
    const std::string path = debug_folder + "/hla_ties.json";
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(text.data(), 1, (size_t)need - 1, f) != (size_t)need - 1) { if (f) std::fclose(f); err = "Error while writing " + path; return SP_ERR_INVALID_ARG; }
    std::fclose(f);
    return SP_OK;
}

// the HLA entries of one sample: PgxMappingDetails of every read, the diplotypes, hla_debug.json.  rec / rev: by position in QNAME order; rev[k].allele
// >= 0 names the reverse-strand mapping a read was dropped for (src/hla/realigner.rs:178-193)
int32_t hla_package(sp_starphase* h, const std::vector<Read4>& reads, const std::vector<uint32_t>& searched, const std::vector<uint32_t>& order,
                    const sp_hla_realign* rec, const sp_hla_rev_hit* rev, const sp_hla_call* calls, const std::string& debug_folder,
                    std::vector<Entry>& out, std::string& err, const ReadCigars* cigars, uint32_t cigars_first,
                    const sp_hla_map* maps = nullptr, const int32_t* map_item = nullptr, std::string* warnings = nullptr,
                    bool want_support = false, const SupportView* support = nullptr) {
    const size_t G = h->hgenes.size();
    // PgxMappingDetails of every read, in the order the loop met them, in the bucket of its gene (realigned) or of the gene searched (ignored)
    std::vector<std::unique_ptr<GeneDetailsPtr>> det(G);
    for (auto& d : det) d.reset(new GeneDetailsPtr());
    std::vector<uint32_t> pos_of(reads.size());
    for (uint32_t k = 0; k < order.size(); ++k) pos_of[order[k]] = k;
    for (uint32_t r = 0; r < reads.size(); ++r) {
        const sp_hla_realign& q = rec[pos_of[r]];
        sp_mapping_stats dna{}; dna.present = 1;
        uint32_t gene = searched[r]; const char* id = "REFERENCE"; std::string star = "REFERENCE"; int32_t ignored = 1;
        const sp_hla_rev_hit& rv = rev[pos_of[r]];
        if (rv.allele >= 0) {                                        // accepted on the reverse strand: ignored, named after that mapping
            const uint32_t a = (uint32_t)rv.allele;
            id = h->a_id[a].c_str(); star = h->hgenes[h->a_gene[a]].name + "*" + h->a_star[a];
            dna.seq_len = (uint64_t)rv.t_len; dna.nm = (uint64_t)rv.nm; dna.unmapped = (uint64_t)(rv.t_len - (rv.t_end - rv.t_start));
        } else if (q.best_allele >= 0 && q.status != 1) {
            const uint32_t a = (uint32_t)q.best_allele;
            id = h->a_id[a].c_str(); star = h->hgenes[h->a_gene[a]].name + "*" + h->a_star[a];
            dna.seq_len = (uint64_t)q.target_len; dna.nm = (uint64_t)q.mm2_nm;
            dna.unmapped = (uint64_t)std::max(0, q.target_len - (q.mm2_t_end - q.mm2_t_start));
            if (q.status == 0) { ignored = 0; gene = h->a_gene[a]; }
        } else { dna.seq_len = reads[r].len; dna.nm = reads[r].len; dna.unmapped = 0; }      // MappingStats::new(read_len, read_len, 0) (realigner.rs:124)
        sp_gene_details_add_mapping(det[gene]->d, reads[r].qname.c_str(), id, star.c_str(), nullptr, &dna, ignored);
    }
    // the diplotypes (src/hla/caller.rs:662-668,889-923,451-474)
    auto name = [&](int32_t a) -> std::string {
        if (a == -2) return ".";
        if (a < 0) return "";
        return "*" + h->a_star[(size_t)a];
    };
    for (size_t g = 0; g < G; ++g) {
        const sp_hla_call& c = calls[g];
        std::string n1, n2;
        if (c.status == 1) n1 = n2 = h->hgenes[g].absent_capable ? "." : "NO_READS";
        else { n1 = name(c.allele1); n2 = name(c.allele2); }
        sp_gene_details_add_diplotype(det[g]->d, n1.c_str(), n2.c_str());
        Entry en; en.gene = h->hgenes[g].name; en.details = std::move(det[g]); en.constructor = SP_DETAILS_FROM_MAPPINGS;
        out.push_back(std::move(en));
    }
    // hla_debug.json: the DualPassingStats of every gene that had reads (src/hla/caller.rs:1042-1048)
    if (!debug_folder.empty()) {
        sp_hla_debug* dbg = nullptr;
        sp_hla_debug_create(&dbg);
        for (size_t g = 0; g < G; ++g) {
            if (calls[g].status == 1) continue;
            for (int k = 0; k < 2; ++k) {
                const int32_t t = k ? calls[g].typed2 : calls[g].typed1;
                if (k == 1 && !calls[g].is_dual) continue;
                const std::string who = k ? "consensus2" : "consensus1";
                const std::string st = t >= 0 ? h->hgenes[h->a_gene[t]].name + "*" + h->a_star[t] : "";
                sp_hla_debug_add_read(dbg, h->hgenes[g].name.c_str(), who.c_str(), t >= 0 ? h->a_id[t].c_str() : nullptr, st.c_str());
                if (h->hla_debug_mappings && maps && map_item && warnings && map_item[g * 2 + k] >= 0) {
                    const int32_t mr = hla_debug_mappings_add(h, dbg, h->hgenes[g].name, who, maps, (uint32_t)map_item[g * 2 + k], *warnings, err);
                    if (mr != SP_OK) { sp_hla_debug_free(dbg); return mr; }
                }
            }
            sp_hla_debug_add_dual_stats(dbg, h->hgenes[g].name.c_str(), &calls[g]);
        }
        const std::string path = debug_folder + "/hla_debug.json";
        const int32_t rc = sp_hla_debug_save(dbg, path.c_str());
        sp_hla_debug_free(dbg);
        if (rc != SP_OK) { err = "Error while writing " + path; return rc; }
        if (cigars) { const int32_t rd = read_debug_save(h, reads, pos_of, rec, *cigars, cigars_first, debug_folder, err); if (rd != SP_OK) return rd; }
        if (want_support) { const int32_t rs = consensus_support_save(h, calls, support, debug_folder, err); if (rs != SP_OK) return rs; }
        if (h->hla_ties) { const int32_t rt = hla_ties_save(h, calls, maps, map_item, debug_folder, err); if (rt != SP_OK) return rt; }
    }
    return SP_OK;
}

// ---------------------------------------------------------------- CYP2D6
struct CypLane {
    bool decoded = false; std::vector<Read4> reads;  // the reads of the extraction region (cyp_decode)
    int32_t rc = SP_OK; std::string err, warnings;
    Entry entry; double decode_ms = 0; uint32_t n_reads = 0;
};

void cyp_problem(sp_starphase* h, sp_cyp_problem& pr) {
    sp_cyp_db_problem(h->cyp, &pr);
    pr.min_consensus_count = (int32_t)h->s.min_consensus_count; pr.dual_max_ed_delta = (int32_t)h->s.dual_max_ed_delta;
    pr.min_consensus_fraction = h->s.min_consensus_fraction; pr.infer_connections = h->s.infer_connections; pr.normalize_d6_only = h->s.normalize_d6_only;
}

// the CYP2D6 entry of a sample whose reads were typed: the call, multi_mapping_details, cyp2d6_alleles.json
void cyp_package(sp_starphase* h, const sp_cyp_problem& pr, const sp_cyp_call& call, const sp_cyp_region_variants& rv, const std::vector<sp_cyp_read_mapping>& mappings,
                 const std::vector<uint32_t>& order, const std::string& debug_folder, const std::string& alternatives, const std::string& alternative_reads, CypLane* L) {
    const std::vector<Read4>& reads = L->reads;
    sp_gene_details* d = L->entry.details->d;
    if (call.status == 16 || call.status == 17 || call.status == 18) {              // CallerError -> PgxGeneDetails::no_match() (src/diplotyper.rs:316-327)
        L->entry.constructor = SP_DETAILS_NO_MATCH;
    } else if (call.status == 1) {
        sp_gene_details_add_diplotype(d, "NO_READS", "NO_READS");
    } else if (call.status != 0) {
        L->rc = SP_ERR_CHAIN_COLLAPSE; L->err = "CYP2D6: chain collapse"; return;
    } else {
        sp_gene_details_add_diplotype(d, call.hap1, call.hap2);
        sp_gene_details_add_simple_diplotype(d, call.core1, call.core2);
        sp_gene_details_add_diplotype_only(d, call.deep1, call.deep2);
        for (const sp_cyp_read_mapping& m : mappings)                               // multi_mapping_details (src/cyp2d6/caller.rs:541-565)
            sp_gene_details_add_multi_mapping(d, reads[order[m.read]].qname.c_str(), m.read_start, m.read_end, m.consensus, m.index_label);
        if (!debug_folder.empty()) {
            uint64_t need = 0;
            sp_cyp_alleles_json(&pr, &call, &rv, nullptr, 0, &need);
            std::string text(need, '\0');
            if (sp_cyp_alleles_json(&pr, &call, &rv, &text[0], need, &need) != SP_OK) { L->rc = SP_ERR_INVALID_ARG; L->err = "cyp2d6_alleles.json"; return; }
            text.resize(std::strlen(text.c_str()));
            const std::string path = debug_folder + "/cyp2d6_alleles.json";
            FILE* f = std::fopen(path.c_str(), "wb");
            if (!f || std::fwrite(text.data(), 1, text.size(), f) != text.size()) { if (f) std::fclose(f); L->rc = SP_ERR_INVALID_ARG; L->err = "Error while writing " + path; return; }
            std::fclose(f);
        }
        if (!debug_folder.empty() && !alternatives.empty()) {                      // sp_starphase_set_cyp_alternatives: the text the chain-pair search left
            const std::string path = debug_folder + "/cyp2d6_alternatives.json";
            FILE* f = std::fopen(path.c_str(), "wb");
            if (!f || std::fwrite(alternatives.data(), 1, alternatives.size(), f) != alternatives.size()) { if (f) std::fclose(f); L->rc = SP_ERR_INVALID_ARG; L->err = "Error while writing " + path; return; }
            std::fclose(f);
        }
        if (!debug_folder.empty() && !alternative_reads.empty()) {                 // sp_starphase_set_cyp_alternative_reads: the same search's pairs read by read
            const std::string path = debug_folder + "/cyp2d6_alternative_reads.json";
            FILE* f = std::fopen(path.c_str(), "wb");
            if (!f || std::fwrite(alternative_reads.data(), 1, alternative_reads.size(), f) != alternative_reads.size()) { if (f) std::fclose(f); L->rc = SP_ERR_INVALID_ARG; L->err = "Error while writing " + path; return; }
            std::fclose(f);
        }
    }
}

// cyp2d6_consensus_support.json of one sample (sp_starphase_set_cyp_consensus_support): the tables of the group's one support pass that belong to this sample
// (off: MAXCONS + 1 offsets into cols, sm: MAXCONS summaries, cons: the sample's consensus block).  A failure fails the sample's CYP2D6 entry.
void cyp_support_save(const sp_cyp_call& call, const char* cons, uint32_t cons_cap, const uint64_t* off, const sp_pileup_col* cols, const sp_support_summary* sm,
                      const SupportLists& lists, uint64_t slot0, const std::string& debug_folder, CypLane* L) {
    const uint64_t n_haps = lists.haps.size();                       // (heads: the pass's, the sample's first at slot0)
    uint64_t need = 0;
    int32_t rc = sp_cyp_support_json_hap(&call, cons, cons_cap, off, cols, sm, lists.ins.data(), lists.ins.size(), n_haps ? lists.haps.data() : nullptr, n_haps, n_haps ? lists.heads.data() : nullptr, slot0,
                                         nullptr, 0, nullptr, 0, nullptr, 0, &need);
    std::string text((size_t)need, '\0');
    if (rc == SP_OK || rc == SP_ERR_CAPACITY) rc = sp_cyp_support_json_hap(&call, cons, cons_cap, off, cols, sm, lists.ins.data(), lists.ins.size(), n_haps ? lists.haps.data() : nullptr, n_haps,
                                                                           n_haps ? lists.heads.data() : nullptr, slot0, nullptr, 0, nullptr, 0, &text[0], need, &need);
    if (rc != SP_OK) { L->rc = rc; L->err = "cyp2d6_consensus_support.json: the tables do not fit their consensuses"; return; }
    const std::string path = debug_folder + "/cyp2d6_consensus_support.json";
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(text.data(), 1, (size_t)need - 1, f) != (size_t)need - 1) { if (f) std::fclose(f); L->rc = SP_ERR_INVALID_ARG; L->err = "Error while writing " + path; return; }
    std::fclose(f);
}

// ---------------------------------------------------------------- the pipeline of a group of samples
struct Sample : VarSample {
    std::vector<std::string> bams; std::string debug; bool run_hla = false, run_cyp = false;
    int stage = 0;                                   // where it failed: 0 the checks, 1 variant genes, 2 HLA, 3 CYP2D6 or the result
    std::string warnings;
    // HLA: decoded (hla_decode), typed
    std::vector<Read4> hreads; std::vector<uint32_t> hsearched; std::string hwarn, herr; int32_t hrc = SP_OK;
    std::vector<Entry> hla_entries;
    CypLane cyp;
    void fail(int at, int32_t code, const std::string& m) { if (rc == SP_OK) { rc = code; err = m; stage = at; } }
};

// the inputs of a sample, resolved against the handle's, and the checks made before anything is read
void sample_setup(sp_starphase* h, const sp_sample_inputs& in, const std::string& debug_folder, Sample& b) {
    for (uint32_t k = 0; k < in.n_bams; ++k) b.bams.push_back(opt(in.bams[k]));
    b.has_vcf = in.vcf != nullptr; b.vcf = opt(in.vcf);
    b.sample = in.sample_name ? opt(in.sample_name) : h->sample_name;
    b.sv = in.sv_vcf ? opt(in.sv_vcf) : h->sv_vcf;
    b.debug = debug_folder;
    if (!b.bams.empty() && !h->fasta) b.fail(0, SP_ERR_INVALID_ARG, "Reference genome is required for reading alignment files");
    else if (!b.bams.empty() && !h->s.debug_skip_hla && !h->hla_err.empty()) b.fail(0, SP_ERR_INVALID_ARG, h->hla_err);
    else if (!b.bams.empty() && h->cyp_selected && !h->cyp_err.empty()) b.fail(0, SP_ERR_INVALID_ARG, h->cyp_err);
    if (b.rc != SP_OK) return;
    b.run_hla = !b.bams.empty() && h->hla && !h->s.debug_skip_hla;
    b.run_cyp = !b.bams.empty() && h->cyp_selected && h->cyp;
    if (!b.debug.empty()) mkdir(b.debug.c_str(), 0755);
}

void hla_decode(sp_starphase* h, Sample& b) { b.hrc = hla_collect(h, b.bams, b.hreads, b.hsearched, b.hwarn, b.herr); }
void cyp_decode(sp_starphase* h, Sample& b) {
    const auto t0 = std::chrono::steady_clock::now();
    CypLane& L = b.cyp;
    std::set<std::string> seen;
    L.rc = collect_reads(b.bams, h->cyp_chrom, h->cyp_start, h->cyp_end, seen, L.reads, L.warnings, L.err);
    L.decoded = true; L.decode_ms = ms_since(t0);
}
// everything a sample reads from its files, ahead of the lanes (a decode worker of a batch)
void decode_sample(sp_starphase* h, Sample& b) {
    if (b.rc != SP_OK) return;
    if (b.has_vcf) vcf_fetch(h, h->win, b.vcf, b.sv, b.sample, b.vf);
    if (b.run_hla) hla_decode(h, b);
    if (b.run_cyp) cyp_decode(h, b);
}

// the CYP2D6 lane of a group, on the second context: a sample not decoded ahead reads its BAMs here (so a single call's decode runs on this lane's thread),
// then one cohort call for the samples with reads -- a lane with one such sample takes the single-sample entry point.
// only_ok (settings.sequential): the samples whose other lanes failed are skipped
void cyp_group(sp_starphase* h, std::vector<Sample*> group, bool only_ok, double* ms) {
    auto t0 = std::chrono::steady_clock::now();
    sp_cyp_problem pr{};
    cyp_problem(h, pr);
    std::vector<Sample*> typed; std::vector<std::vector<uint32_t>> orders; std::vector<sp_seqset*> sets;
    for (Sample* b : group) {
        if (!b->run_cyp || (only_ok && b->rc != SP_OK)) continue;
        CypLane* L = &b->cyp;
        L->entry.gene = "CYP2D6"; L->entry.details.reset(new GeneDetailsPtr());
        if (!L->decoded) cyp_decode(h, *b);
        L->n_reads = (uint32_t)L->reads.size();
        if (L->rc != SP_OK) continue;
        L->entry.constructor = SP_DETAILS_FROM_MULTI_MAPPINGS;
        // "No reads found for CYP2D6 consensus generation." (src/cyp2d6/caller.rs:254-266)
        if (L->reads.empty()) { sp_gene_details_add_diplotype(L->entry.details->d, "NO_READS", "NO_READS"); continue; }
        orders.push_back(qname_order(L->reads));                     // read_collection is a BTreeMap: QNAME order
        sp_seqset* set = nullptr;
        const int32_t rc = upload_reads(h->ctx2, {{&L->reads, &orders.back()}}, &set);
        if (rc != SP_OK) { L->rc = rc; L->err = "read upload: " + opt(sp_last_error(h->ctx2)); orders.pop_back(); continue; }
        typed.push_back(b); sets.push_back(set);
    }
    const uint32_t n = (uint32_t)typed.size();
    if (n) {
        std::vector<sp_cyp_call> calls(n);
        const size_t per = (size_t)SP_CYP_MAXCONS * std::max<uint32_t>(pr.n_variants, 1);
        std::vector<uint8_t> state(per * n);
        std::vector<sp_cyp_region_variants> rv(n);
        for (uint32_t k = 0; k < n; ++k) { rv[k] = sp_cyp_region_variants{}; rv[k].state = state.data() + per * k; }
        std::vector<std::vector<sp_cyp_read_mapping>> mappings(n);
        std::vector<int32_t> rcs(n, SP_ERR_INVALID_ARG);             // until the cohort call has typed it
        // cyp2d6_alternatives.json (sp_starphase_set_cyp_alternatives): the samples with a debug folder run the N-best form of the chain-pair search, which leaves the text
        std::vector<std::string> alts(n); std::vector<std::string*> alt_of(n, nullptr); bool want_alts = false;
        for (uint32_t k = 0; k < n; ++k) if (h->cyp_alternatives && !typed[k]->debug.empty()) { alt_of[k] = &alts[k]; want_alts = true; }
        // cyp2d6_alternative_reads.json (sp_starphase_set_cyp_alternative_reads): the same search, then its pairs read by read; the QNAMEs in the order of the sample's set
        std::vector<SpiCypAltReads> areads(n); std::vector<SpiCypAltReads*> aread_of(n, nullptr); std::vector<std::vector<const char*>> qnames(n); bool want_areads = false;
        for (uint32_t k = 0; k < n; ++k) if (h->cyp_alternative_reads && !typed[k]->debug.empty()) {
            for (uint32_t i : orders[k]) qnames[k].push_back(typed[k]->cyp.reads[i].qname.c_str());
            areads[k].read_names = qnames[k].data(); aread_of[k] = &areads[k]; want_areads = true;
        }
        // cyp2d6_consensus_support.json: the calls also hand out their consensuses (the calls themselves are the same), for one support pass over the group below
        // cyp2d6_alleles.vcf.gz (sp_starphase_set_cyp_vcf) takes its SR / CR from the same pass: want_support is "the pass runs", want_json / want_vcf say what is written
        bool want_json = false, want_vcf = false;
        for (uint32_t k = 0; k < n; ++k) { want_json |= h->cyp_consensus_support && !typed[k]->debug.empty(); want_vcf |= h->cyp_vcf && !typed[k]->debug.empty(); }
        const bool want_support = want_json || want_vcf;
        // (a consensus has at most 65,534 bases, like a read; the block is SP_CYP_MAXCONS x that = 4 MB of host memory per sample of the group while the lane runs,
        //  256 MB for a group of 64: sized by the limit, not by the reads, because a consensus over offset reads may be longer than any one of its segments)
        const uint32_t cons_cap = want_support ? 65536u : 0u;
        const size_t cons_block = (size_t)SP_CYP_MAXCONS * cons_cap;
        std::vector<char> cons(want_support ? cons_block * n : 0, '\0');
        char* cons_out = want_support ? cons.data() : nullptr;
        if (n > 1) spi_cyp_diplotype_cohort_mappings(h->ctx2, &pr, n, sets.data(), calls.data(), cons_out, cons_cap, rv.data(), mappings.data(), rcs.data(), want_alts ? alt_of.data() : nullptr,
                                                     want_areads ? aread_of.data() : nullptr);
        std::vector<uint8_t> packaged(n, 0);
        for (uint32_t k = 0; k < n; ++k) {
            CypLane* L = &typed[k]->cyp;
            if (rcs[k] != SP_OK) {
                // alone: the only sample of the lane, or one the cohort call failed (the context's error text may be another sample's)
                const int32_t rc = spi_cyp_diplotype_mappings(h->ctx2, &pr, sets[k], &calls[k], cons_out ? cons_out + cons_block * k : nullptr, cons_cap, &rv[k], &mappings[k], alt_of[k], aread_of[k]);
                if (rc != SP_OK) { L->rc = rc; L->err = "sp_cyp_diplotype: " + opt(sp_last_error(h->ctx2)); continue; }
            }
            cyp_package(h, pr, calls[k], rv[k], mappings[k], orders[k], typed[k]->debug, alts[k], areads[k].text, L);
            packaged[k] = L->rc == SP_OK;
        }
        if (want_support) {
            // one pass over the samples that have a debug folder and a call (status 0: the others write no file); the others are handed over as failed calls, which own nothing
            std::vector<sp_cyp_call> sc(calls); std::vector<sp_cyp_read_mapping> flat; std::vector<uint64_t> moff(n + 1, 0); std::vector<uint32_t> on;
            uint64_t n_cols = 0;
            for (uint32_t k = 0; k < n; ++k) {
                const bool take = packaged[k] && !typed[k]->debug.empty() && calls[k].status == 0;
                if (take) {
                    on.push_back(k); flat.insert(flat.end(), mappings[k].begin(), mappings[k].end());
                    for (int32_t x = 0; x < calls[k].n_consensus && x < SP_CYP_MAXCONS; ++x) n_cols += strnlen(cons.data() + cons_block * k + (size_t)x * cons_cap, cons_cap);
                } else sc[k].status = -1;
                moff[k + 1] = flat.size();
            }
            if (!on.empty()) {
                if (!want_json) n_cols = 0;                          // (the table is not downloaded for the VCF alone)
                std::vector<uint64_t> off((size_t)n * SP_CYP_MAXCONS + 1, 0); std::vector<sp_pileup_col> cols((size_t)n_cols + 1); std::vector<sp_support_summary> sm((size_t)n * SP_CYP_MAXCONS);
                sp_pileup_col* cols_out = want_json ? cols.data() : nullptr;
                // the variant support of the group (want_vcf): SP_CYP_MAXCONS * n_variants records per sample, from the windows the pass counts
                const size_t vper = (size_t)SP_CYP_MAXCONS * pr.n_variants;
                std::vector<sp_window_support> vsup(want_vcf ? std::max<size_t>(vper * n, 1) : 0); std::vector<int32_t> vok(want_vcf ? std::max<size_t>(vper * n, 1) : 0);
                const CypVariantIn vin = { &pr, rv.data(), SP_CYP_VCF_FLANK, vsup.data(), vok.data() };
                auto vcf_save = [&](uint32_t k, const sp_window_support* sup, const int32_t* ok, CypLane* L) {
                    if (!want_vcf || L->rc != SP_OK) return;
                    const std::string path = typed[k]->debug + "/cyp2d6_alleles.vcf.gz";
                    const int32_t rc_v = sp_cyp_alleles_vcf_save(h->cyp, &calls[k], &rv[k], sup, ok, nullptr, nullptr, path.c_str());
                    if (rc_v != SP_OK) { L->rc = rc_v; L->err = "Error while writing " + path; }
                };
                SupportLists lists;                                  // (stay empty without sp_starphase_set_support_insertions / _haplotypes: the renderer then writes the file as before)
                const bool want_ins = h->support_insertions != 0, want_haps = h->support_haplotypes != 0;
                int32_t rc = support_with_lists(lists, want_ins, want_haps, (size_t)n * SP_CYP_MAXCONS, [&](sp_pileup_ins* p, uint64_t room, uint64_t* got, sp_support_hap* hp, uint64_t hroom, uint64_t* hgot, sp_support_hap_head* hd) {
                    return spi_cyp_support_cohort(h->ctx2, n, sets.data(), sc.data(), cons.data(), cons_cap, flat.data(), moff.data(), off.data(), cols_out, n_cols, sm.data(), p, room, got, hp, hroom, hgot, hd,
                                                  want_vcf ? &vin : nullptr); });
                if (rc == SP_OK) {
                    for (uint32_t k : on) {
                        if (want_json) cyp_support_save(calls[k], cons.data() + cons_block * k, cons_cap, off.data() + (size_t)k * SP_CYP_MAXCONS, cols.data(), sm.data() + (size_t)k * SP_CYP_MAXCONS, lists, (uint64_t)k * SP_CYP_MAXCONS, typed[k]->debug, &typed[k]->cyp);
                        vcf_save(k, vsup.data() + vper * k, vok.data() + vper * k, &typed[k]->cyp);
                    }
                } else for (uint32_t k : on) {
                    // the shared pass failed: sample by sample, and only the samples whose own pass fails are failed (alone in the pass: that failure is its own)
                    CypLane* L = &typed[k]->cyp;
                    if (on.size() > 1) rc = support_with_lists(lists, want_ins, want_haps, SP_CYP_MAXCONS, [&](sp_pileup_ins* p, uint64_t room, uint64_t* got, sp_support_hap* hp, uint64_t hroom, uint64_t* hgot, sp_support_hap_head* hd) {
                        const uint64_t moff1[2] = { 0, mappings[k].size() };
                        const CypVariantIn vin1 = { &pr, &rv[k], SP_CYP_VCF_FLANK, vsup.data(), vok.data() };
                        return spi_cyp_support_cohort(h->ctx2, 1, &sets[k], &calls[k], cons.data() + cons_block * k, cons_cap, mappings[k].data(), moff1, off.data(), cols_out, n_cols, sm.data(), p, room, got, hp, hroom, hgot, hd,
                                                      want_vcf ? &vin1 : nullptr); });
                    if (rc != SP_OK) { L->rc = rc; L->err = "sp_cyp_consensus_support: " + opt(sp_last_error(h->ctx2)); continue; }
                    if (want_json) cyp_support_save(calls[k], cons.data() + cons_block * k, cons_cap, off.data(), cols.data(), sm.data(), lists, 0, typed[k]->debug, L);
                    vcf_save(k, on.size() > 1 ? vsup.data() : vsup.data() + vper * k, on.size() > 1 ? vok.data() : vok.data() + vper * k, L);
                }
            }
        }
    }
    for (sp_seqset* s : sets) sp_seqset_free(s);
    *ms += ms_since(t0);
}

// the HLA lane of samples that share the device passes: their reads in one set (sample by sample, QNAME order within a sample; each read is realigned
// by itself, so any order gives the same records), one K1 pass that also names the reverse-strand reads, the (sample, gene) problems in one call
// (the single-sample entry point when one sample has reads), then each sample's entries.
// Exhaustive K1 (a caller's context with k1_best_n = 0) has no seeded stage to take reverse-strand mappings from: no read is named after one.
int32_t hla_pass(sp_starphase* h, const std::vector<Sample*>& with, std::string& err) {
    const size_t G = h->hgenes.size();
    const uint32_t cap = 1 << 16;
    std::vector<std::vector<uint32_t>> orders; std::vector<uint32_t> first{0}; std::vector<ReadPart> parts;
    for (Sample* b : with) { orders.push_back(qname_order(b->hreads)); first.push_back(first.back() + (uint32_t)b->hreads.size()); }
    for (size_t k = 0; k < with.size(); ++k) parts.push_back(ReadPart{&with[k]->hreads, &orders[k]});
    const uint32_t R = first.back();
    std::vector<sp_hla_realign> rec(R); std::vector<sp_hla_rev_hit> rev(R, sp_hla_rev_hit{-1, 0, 0, 0, 0, 0});
    std::vector<sp_hla_call> calls(with.size() * G);
    for (auto& c : calls) { std::memset(&c, 0, sizeof c); c.status = 1; }
    bool want_cigars = false;                                        // one traceback pass for the group when any of its samples has a debug folder
    for (Sample* b : with) want_cigars |= h->read_debug && !b->debug.empty();
    ReadCigars cigars; cigars.stride = 1;
    bool want_maps = false;                                          // likewise one batched map of the group's consensuses
    for (Sample* b : with) want_maps |= (h->hla_debug_mappings || h->hla_ties) && !b->debug.empty();
    HlaMaps maps; std::vector<int32_t> map_item(with.size() * G * 2, -1);
    bool want_support = false;                                       // likewise one support pass (anchor, alignment, pileup) over the group's consensuses
    for (Sample* b : with) want_support |= h->consensus_support && !b->debug.empty();
    std::vector<uint8_t> is1; std::vector<uint64_t> sup_off; std::vector<sp_pileup_col> sup_cols; std::vector<sp_support_summary> sup_sm;
    SupportLists sup_lists;                                          // (sp_starphase_set_support_insertions / _haplotypes; empty otherwise)
    std::vector<int32_t> cohort_of(with.size(), -1);                 // a sample's place among the samples with reads
    if (R) {
        sp_seqset* set = nullptr;
        int32_t rc = upload_reads(h->ctx, parts, &set);
        if (rc != SP_OK) { err = "read upload: " + opt(sp_last_error(h->ctx)); return rc; }
        std::unique_ptr<sp_seqset, void (*)(sp_seqset*)> guard(set, sp_seqset_free);
        rc = h->ctx->k1_best_n > 0 ? sp_hla_realign_reads_rev(h->ctx, h->hla, set, rec.data(), rev.data()) : sp_hla_realign_reads(h->ctx, h->hla, set, rec.data(), nullptr);
        if (rc != SP_OK) { err = "sp_hla_realign_reads: " + opt(sp_last_error(h->ctx)); return rc; }
        // the samples with reads are the cohort; a sample without reads keeps the no-reads calls
        std::vector<uint32_t> read_sample(R), at;
        std::vector<sp_hla_call_config> cfg;
        for (size_t k = 0; k < with.size(); ++k) {
            if (first[k + 1] == first[k]) continue;
            for (uint32_t r = first[k]; r < first[k + 1]; ++r) read_sample[r] = (uint32_t)at.size();
            cohort_of[k] = (int32_t)at.size();
            at.push_back((uint32_t)k);
            cfg.resize(at.size() * G);
            hla_configs(h, rec.data() + first[k], first[k + 1] - first[k], cfg.data() + (at.size() - 1) * G);
        }
        std::vector<uint32_t> genes(G);
        for (size_t g = 0; g < G; ++g) genes[g] = (uint32_t)g;
        std::vector<sp_hla_call> cc(at.size() * G);
        const size_t need = at.size() * G * 2 * (size_t)cap;
        if (h->hla_cons.size() < need) h->hla_cons.resize(need);
        if (want_support) is1.assign(R, 0);
        uint8_t* is1_out = want_support ? is1.data() : nullptr;
        rc = at.size() == 1 ? sp_hla_diplotype_genes(h->ctx, h->hla, (uint32_t)G, genes.data(), set, rec.data(), cfg.data(), cc.data(), h->hla_cons.data(), cap, is1_out)
                            : sp_hla_diplotype_cohort_samples(h->ctx, h->hla, (uint32_t)at.size(), read_sample.data(), (uint32_t)G, genes.data(), set, rec.data(),
                                                              cfg.data(), cc.data(), h->hla_cons.data(), cap, is1_out);
        if (rc != SP_OK) { err = "sp_hla_diplotype_genes: " + opt(sp_last_error(h->ctx)); return rc; }
        for (size_t x = 0; x < at.size(); ++x) std::copy(cc.begin() + x * G, cc.begin() + (x + 1) * G, calls.begin() + (size_t)at[x] * G);
        if (want_cigars) { rc = read_cigars(h, set, rec.data(), R, &cigars, err); if (rc != SP_OK) return rc; }
        // consensus_support.json: the member reads of every called gene of the samples that have a debug folder, piled under their consensuses in one pass
        if (want_support) {
            std::vector<uint8_t> unit_on(at.size() * G, 0);
            uint64_t n_cols = 0;
            for (size_t x = 0; x < at.size(); ++x) {
                if (with[at[x]]->debug.empty()) continue;
                for (size_t g = 0; g < G; ++g) {
                    if (cc[x * G + g].status == 1) continue;
                    unit_on[x * G + g] = 1;
                    for (int k = 0; k < 2; ++k) n_cols += strnlen(h->hla_cons.data() + ((x * G + g) * 2 + k) * (size_t)cap, cap);
                }
            }
            sup_off.assign(at.size() * G * 2 + 1, 0); sup_cols.resize((size_t)n_cols + 1); sup_sm.resize(at.size() * G * 2);
            rc = support_with_lists(sup_lists, h->support_insertions != 0, h->support_haplotypes != 0, at.size() * G * 2, [&](sp_pileup_ins* p, uint64_t room, uint64_t* got, sp_support_hap* hp, uint64_t hroom, uint64_t* hgot, sp_support_hap_head* hd) {
                return sp_hla_consensus_support_cohort_hap(h->ctx, h->hla, (uint32_t)at.size(), read_sample.data(), (uint32_t)G, genes.data(), set, rec.data(), is1.data(),
                                                           h->hla_cons.data(), cap, unit_on.data(), sup_off.data(), sup_cols.data(), n_cols, sup_sm.data(), p, room, got, hp, hroom, hgot, hd); });
            if (rc != SP_OK) { err = "sp_hla_consensus_support: " + opt(sp_last_error(h->ctx)); return rc; }
        }
        // the per-allele mappings of hla_debug.json: every consensus of the samples that have a debug folder, in one batched map
        if (want_maps) {
            std::vector<uint32_t> mg, ml, where; std::vector<const char*> mc;
            for (size_t x = 0; x < at.size(); ++x) {
                if (with[at[x]]->debug.empty()) continue;
                for (size_t g = 0; g < G; ++g) {
                    const sp_hla_call& c = cc[x * G + g];
                    if (c.status == 1) continue;
                    for (int k = 0; k < 2; ++k) {
                        if (k == 1 && !c.is_dual) continue;
                        const char* cons = h->hla_cons.data() + ((x * G + g) * 2 + k) * (size_t)cap;
                        const size_t len = strnlen(cons, cap);
                        if (!len) continue;
                        mg.push_back((uint32_t)g); mc.push_back(cons); ml.push_back((uint32_t)len); where.push_back((uint32_t)(((size_t)at[x] * G + g) * 2 + k));
                    }
                }
            }
            if (!mg.empty()) {
                std::vector<uint32_t> item_of;
                rc = spi_hla_map_type_batch(h->ctx, h->hla, (uint32_t)mg.size(), mg.data(), mc.data(), ml.data(), h->s.hla_require_dna, h->s.disable_cdna_scoring, &maps.map, &item_of,
                                            h->hla_ties ? SP_HLA_MAP_TIES : 0u);
                if (rc != SP_OK) { err = "sp_hla_map_type_consensus: " + opt(sp_last_error(h->ctx)); return rc; }
                for (size_t i = 0; i < item_of.size(); ++i) map_item[where[item_of[i]]] = (int32_t)i;
            }
        }
    }
    for (size_t k = 0; k < with.size(); ++k) {
        Sample* b = with[k];
        std::string e;
        SupportView sv{};
        const bool sup = want_support && cohort_of[k] >= 0 && !sup_off.empty();
        if (sup) { const size_t x = (size_t)cohort_of[k]; sv = SupportView{ sup_off.data() + x * G * 2, sup_cols.data(), sup_sm.data() + x * G * 2, h->hla_cons.data() + x * G * 2 * (size_t)cap, cap, sup_lists.ins.data(), sup_lists.ins.size(),
                                                                            sup_lists.haps.data(), sup_lists.haps.size(), sup_lists.heads.data(), sup_lists.heads.size(), x * G * 2 }; }
        const int32_t rc = hla_package(h, b->hreads, b->hsearched, orders[k], rec.data() + first[k], rev.data() + first[k], calls.data() + k * G, b->debug, b->hla_entries, e,
                                       want_cigars ? &cigars : nullptr, first[k], maps.map, maps.map ? map_item.data() + k * G * 2 : nullptr, &b->hwarn,
                                       h->consensus_support != 0, sup ? &sv : nullptr);
        if (rc != SP_OK) b->fail(2, rc, e);
    }
    return SP_OK;
}

// the HLA lane of a group (decoded already); returns the reads it typed.  The shared passes fail as a whole (a read too long for K1, a failing consensus
// unit of one sample, ...): the group then goes through them once more sample by sample, so only the sample that has the failure fails, with its own text
uint64_t hla_group(sp_starphase* h, const std::vector<Sample*>& group) {
    std::vector<Sample*> with; uint64_t n_reads = 0;
    for (Sample* b : group) {
        if (!b->run_hla || b->rc != SP_OK) continue;
        if (b->hrc != SP_OK) { b->fail(2, b->hrc, b->herr); continue; }
        n_reads += b->hreads.size();
        with.push_back(b);
    }
    if (with.empty()) return n_reads;
    std::string err;
    const int32_t rc = hla_pass(h, with, err);
    if (rc == SP_OK) return n_reads;
    if (with.size() == 1) { with[0]->fail(2, rc, err); return n_reads; }
    for (Sample* b : with) {
        b->hla_entries.clear();
        std::string e;
        const int32_t rb = hla_pass(h, {b}, e);
        if (rb != SP_OK) b->fail(2, rb, e);
    }
    return n_reads;
}

// the result of a sample whose lanes are done.  Errors in the order the checks, variant genes, HLA, CYP2D6, the result itself; the warnings are the HLA
// lane's if it ran and the CYP2D6 lane's only if everything before it succeeded.  The entries in the reference's order: variant genes, HLA genes, CYP2D6
// (StarphaseJson::insert refuses a second entry for a gene).  Gives the sample's reads and entries back.
void sample_result(sp_starphase* h, Sample& b, sp_result** out) {
    if (b.rc == SP_OK && b.run_cyp && b.cyp.rc != SP_OK) b.fail(3, b.cyp.rc, b.cyp.err);
    const bool hla_ran = b.rc == SP_OK || b.stage >= 2, cyp_kept = b.rc == SP_OK || b.stage >= 3;
    b.warnings = (hla_ran ? b.hwarn : std::string()) + (cyp_kept && b.run_cyp ? b.cyp.warnings : std::string());
    if (b.rc == SP_OK) {
        sp_result* res = nullptr;
        sp_result_create(h->db, nullptr, &res);
        std::unique_ptr<sp_result, void (*)(sp_result*)> guard(res, sp_result_free);
        std::vector<Entry*> all;
        for (auto& e : b.entries) all.push_back(&e);
        for (auto& e : b.hla_entries) all.push_back(&e);
        if (b.run_cyp) all.push_back(&b.cyp.entry);
        for (Entry* e : all)
            if (b.rc == SP_OK && sp_result_insert(res, e->gene.c_str(), e->details->d, e->constructor) != SP_OK) b.fail(3, SP_ERR_INVALID_ARG, opt(sp_result_last_error(res)));
        if (b.rc == SP_OK) *out = guard.release();
    }
    std::vector<Read4>().swap(b.hreads); std::vector<uint32_t>().swap(b.hsearched); std::vector<Read4>().swap(b.cyp.reads); b.vf = VcfFetch();
    b.entries.clear(); b.hla_entries.clear(); b.cyp.entry.details.reset();
}

}  // namespace

extern "C" {

void sp_diplotype_settings_default(sp_diplotype_settings* s) {
    if (!s) return;
    std::memset(s, 0, sizeof *s);
    s->max_sv_length = 1000000; s->max_error_rate = 0.07; s->min_cdf_prob = 0.001; s->expected_maf = 0.45;
    s->min_consensus_fraction = 0.10; s->min_consensus_count = 3; s->dual_max_ed_delta = 100;
}

// check_diplotype_settings (src/cli/diplotype.rs:200-330), messages as the reference's
int32_t sp_diplotype_settings_check(sp_diplotype_settings* s, const sp_sample_inputs* in, char* err, uint32_t err_cap) {
    auto fail = [&](const char* m) { if (err && err_cap) { std::snprintf(err, err_cap, "%s", m); } return (int32_t)SP_ERR_INVALID_ARG; };
    if (err && err_cap) err[0] = 0;
    if (!s) return fail("no settings");
    const bool has_vcf = in && in->vcf, has_bam = in && in->n_bams > 0;
    if (!has_vcf && !has_bam) return fail("Must provide a VCF file and/or aligned BAM file to perform diplotyping.");
    if (s->include_set && s->exclude_set) return fail("Only one of --exclude-set and --include-set can be specified.");
    if (has_bam) {
        if (s->disable_cdna_scoring) s->hla_require_dna = 1;                 // "Automatically enabling HLA DNA requirement"
        if (!(s->max_error_rate >= 0.0 && s->max_error_rate <= 1.0)) return fail("--max-error-rate must be between 0.0 and 1.0");
        if (!(s->min_cdf_prob >= 0.0 && s->min_cdf_prob <= 1.0)) return fail("--min-cdf-prob must be between 0.0 and 1.0");
        if (!(s->expected_maf >= 0.01 && s->expected_maf <= 0.5)) return fail("--expected-maf must be between 0.01 and 0.5");
        if (!(s->min_consensus_fraction >= 0.0 && s->min_consensus_fraction <= 1.0)) return fail("--min-consensus-fraction must be between 0.0 and 1.0");
    }
    return SP_OK;
}

void sp_starphase_free(sp_starphase* h) {
    if (!h) return;
    for (auto& v : h->vgenes) sp_variant_gene_free(v.g);
    if (h->hla) sp_hla_db_free(h->hla);
    if (h->cyp) sp_cyp_db_free(h->cyp);
    if (h->fasta) sp_fasta_free(h->fasta);
    if (h->db) sp_database_free(h->db);
    if (h->ctx2) sp_ctx_destroy(h->ctx2);
    if (h->own_ctx && h->ctx) sp_ctx_destroy(h->ctx);
    delete h;
}

const char* sp_starphase_last_error(const sp_starphase* h) { return h ? h->err.c_str() : g_create_error.c_str(); }
const char* sp_starphase_warnings(const sp_starphase* h) { return h ? h->warnings.c_str() : ""; }
int32_t sp_starphase_set_hla_debug_mappings(sp_starphase* h, int32_t on) {
    if (!h) return SP_ERR_INVALID_ARG;
    h->hla_debug_mappings = on ? 1 : 0;
    return SP_OK;
}
int32_t sp_starphase_set_hla_ties(sp_starphase* h, int32_t on) {
    if (!h) return SP_ERR_INVALID_ARG;
    h->hla_ties = on ? 1 : 0;
    return SP_OK;
}
int32_t sp_starphase_set_consensus_support(sp_starphase* h, int32_t on) {
    if (!h) return SP_ERR_INVALID_ARG;
    h->consensus_support = on ? 1 : 0;
    return SP_OK;
}
int32_t sp_starphase_set_cyp_alternatives(sp_starphase* h, int32_t on) {
    if (!h) return SP_ERR_INVALID_ARG;
    h->cyp_alternatives = on ? 1 : 0;
    return SP_OK;
}
int32_t sp_starphase_set_variant_alternatives(sp_starphase* h, int32_t on) {
    if (!h) return SP_ERR_INVALID_ARG;
    h->variant_alternatives = on ? 1 : 0;
    return SP_OK;
}
int32_t sp_starphase_set_cyp_alternative_reads(sp_starphase* h, int32_t on) {
    if (!h) return SP_ERR_INVALID_ARG;
    h->cyp_alternative_reads = on ? 1 : 0;
    return SP_OK;
}
int32_t sp_starphase_set_cyp_vcf(sp_starphase* h, int32_t on) {
    if (!h) return SP_ERR_INVALID_ARG;
    h->cyp_vcf = on ? 1 : 0;
    return SP_OK;
}

int32_t sp_starphase_set_cyp_consensus_support(sp_starphase* h, int32_t on) {
    if (!h) return SP_ERR_INVALID_ARG;
    h->cyp_consensus_support = on ? 1 : 0;
    return SP_OK;
}
int32_t sp_starphase_set_support_haplotypes(sp_starphase* h, int32_t on) {
    if (!h) return SP_ERR_INVALID_ARG;
    h->support_haplotypes = on ? 1 : 0;
    return SP_OK;
}
int32_t sp_starphase_set_support_insertions(sp_starphase* h, int32_t on) {
    if (!h) return SP_ERR_INVALID_ARG;
    h->support_insertions = on ? 1 : 0;
    return SP_OK;
}
int32_t sp_starphase_set_read_debug(sp_starphase* h, int32_t enable) {
    if (!h) return SP_ERR_INVALID_ARG;
    h->read_debug = enable ? 1 : 0;
    return SP_OK;
}
int32_t sp_starphase_last_timing(const sp_starphase* h, sp_starphase_timing* out) {
    if (!h || !out) return SP_ERR_INVALID_ARG;
    *out = h->timing;
    return SP_OK;
}

int32_t sp_starphase_create(sp_ctx* ctx, const char* database_path, const char* reference_fasta, const sp_diplotype_settings* settings, sp_starphase** out) {
    g_create_error.clear();
    if (!out || !database_path || !settings) { g_create_error = "sp_starphase_create: missing argument"; return SP_ERR_INVALID_ARG; }
    *out = nullptr;
    std::unique_ptr<sp_starphase, void (*)(sp_starphase*)> h(new sp_starphase(), sp_starphase_free);
    auto fail = [&](int32_t rc, const std::string& m) { g_create_error = m; return rc; };
    // the two contexts first: no device is an error before any file is read
    h->ctx = ctx;
    if (!ctx) {
        const int32_t rc = sp_ctx_create(0, nullptr, &h->ctx);
        if (rc != SP_OK) return fail(rc, "sp_starphase_create: no usable HIP device");
        h->own_ctx = true;
    }
    sp_ctx_info info{};
    sp_ctx_get_info(h->ctx, &info);
    if (sp_ctx_create(info.device, nullptr, &h->ctx2) != SP_OK) return fail(SP_ERR_NO_DEVICE, "sp_starphase_create: no second context on the device");
    h->s = *settings;
    h->include_set = opt(settings->include_set); h->exclude_set = opt(settings->exclude_set); h->sample_name = opt(settings->sample_name);
    h->sv_vcf = opt(settings->sv_vcf); h->debug_folder = opt(settings->debug_folder);
    h->s.include_set = h->s.exclude_set = h->s.sample_name = h->s.sv_vcf = h->s.debug_folder = nullptr;
    if (settings->include_set && settings->exclude_set) return fail(SP_ERR_INVALID_ARG, "Only one of --exclude-set and --include-set can be specified.");
    if (!h->include_set.empty()) { h->has_include = true; if (!read_lines(h->include_set, h->include)) return fail(SP_ERR_INVALID_ARG, "Include set does not exist: \"" + h->include_set + "\""); }
    if (!h->exclude_set.empty()) { h->has_exclude = true; if (!read_lines(h->exclude_set, h->exclude)) return fail(SP_ERR_INVALID_ARG, "Exclude set does not exist: \"" + h->exclude_set + "\""); }
    char e[1024] = {0};
    if (sp_database_load(database_path, &h->db, e, sizeof e) != SP_OK) return fail(SP_ERR_INVALID_ARG, std::string("Error while loading PGx database file: ") + e);
    if (reference_fasta && sp_fasta_open(reference_fasta, &h->fasta, e, sizeof e) != SP_OK)
        return fail(SP_ERR_INVALID_ARG, std::string("Error while loading reference genome file: ") + e);
    sp_database_stats st{};
    sp_database_info(h->db, &st);
    // variant genes: load_database_haplotypes once per gene (key order)
    for (uint32_t i = 0; i < st.n_gene_entries; ++i) {
        const char* name = nullptr; const char* chrom = nullptr;
        sp_database_gene_entry(h->db, i, &name, &chrom);
        sp_starphase::VGene vg; vg.name = name; vg.chrom = chrom; vg.selected = h->selected(vg.name);
        const char* seq = nullptr; uint64_t len = 0;
        if (h->fasta && !(seq = chrom_bases(h.get(), vg.chrom, &len)))
            return fail(SP_ERR_INVALID_ARG, vg.name + ": Reference genome does not contain contig \"" + vg.chrom + "\"");
        if (sp_variant_gene_create(h->db, name, seq, len, &vg.g) != SP_OK) return fail(SP_ERR_INVALID_ARG, vg.name + ": " + opt(sp_database_last_error(h->db)));
        spi_gene_entry_extras(h->db, vg.g, &vg.reference_allele, &vg.has_sv, &vg.sv_chrom);
        h->vgenes.push_back(std::move(vg));
    }
    // the fetch window of every selected gene with variants (vcf_fetch: +-50 bp around each variant)
    h->win.assign(h->vgenes.size(), GeneWindow());
    for (size_t i = 0; i < h->vgenes.size(); ++i) {
        const sp_starphase::VGene& vg = h->vgenes[i];
        sp_variant_gene_stats st{};
        sp_variant_gene_info(vg.g, &st);
        h->win[i].fetch = vg.selected && !(st.n_variants == 0 && !vg.has_sv); h->win[i].n_variants = st.n_variants;
        uint64_t lo = UINT64_MAX, hi = 0;
        for (uint32_t v = 0; v < st.n_variants; ++v) {
            uint64_t pos; const char *r, *a, *nm, *dbsnp; int64_t vid; int32_t core;
            sp_variant_gene_variant(vg.g, v, &pos, &r, &a, &nm, &dbsnp, &vid, &core);
            lo = std::min(lo, pos > 50 ? pos - 50 : 0); hi = std::max(hi, pos + std::strlen(r) + 51);
        }
        h->win[i].lo = lo; h->win[i].hi = hi;
    }
    if (!h->fasta) { *out = h.release(); return SP_OK; }          // no genome: the BAM loci cannot run (sp_starphase_call says so)
    // HLA: the hla_config genes that are selected, flattened against the reference (+-100 bp, src/hla/realigner.rs:74-81).  The reference builds
    // its realigner only when a sample has BAMs: a locus that cannot be set up here (its contig is not in the FASTA, ...) fails the first call with BAMs
    auto setup_hla = [&]() -> int32_t {
        std::vector<std::string> names, refs;
        for (uint32_t g = 0; g < st.n_hla_genes; ++g) {
            sp_gene_region r{};
            sp_database_hla_gene(h->db, g, &r);
            if (!h->selected(r.name)) continue;
            const char* b = nullptr; uint64_t n = 0;
            const uint64_t lo = r.start >= 100 ? r.start - 100 : 0;
            if (sp_fasta_fetch(h->fasta, r.chrom, lo, r.end + 100, &b, &n) != SP_OK)
                return fail(SP_ERR_INVALID_ARG, std::string(r.name) + ": " + opt(sp_fasta_last_error(h->fasta)));
            names.push_back(r.name); refs.emplace_back(b, n);
            h->hgenes.push_back(sp_starphase::HGene{r.name, r.chrom, r.start, r.end, r.is_absent_capable != 0});
        }
        if (!names.empty()) {
            std::vector<const char*> pn, pr;
            for (size_t i = 0; i < names.size(); ++i) { pn.push_back(names[i].c_str()); pr.push_back(refs[i].c_str()); }
            sp_hla_db_desc desc{};
            if (sp_database_hla_flatten(h->db, (uint32_t)names.size(), pn.data(), pr.data(), 100, &desc) != SP_OK)
                return fail(SP_ERR_INVALID_ARG, "HLA: " + opt(sp_database_last_error(h->db)));
            for (uint32_t a = 0; a < desc.n_alleles; ++a) {
                const char *id, *gene, *star;
                sp_database_hla_allele(h->db, a, &id, &gene, &star);
                h->a_id.push_back(id); h->a_star.push_back(star); h->a_gene.push_back(desc.gene_of[a]);
            }
            const int32_t rc = sp_hla_db_create(h->ctx, &desc, &h->hla);
            if (rc != SP_OK) return fail(rc, "sp_hla_db_create: " + opt(sp_last_error(h->ctx)));
        }
        return SP_OK;
    };
    // CYP2D6: the window of the configuration, the templates and tables on the second context
    h->cyp_selected = h->selected("CYP2D6");
    auto setup_cyp = [&]() -> int32_t {
        const char* chrom = nullptr; uint64_t ws = 0, we = 0;
        if (sp_database_cyp_window(h->db, &chrom, &ws, &we) != SP_OK) return fail(SP_ERR_INVALID_ARG, "CYP2D6: " + opt(sp_database_last_error(h->db)));
        h->cyp_chrom = chrom;
        // the templates reach past the configured coordinates (the *5 signature takes flanks around the deletion): the window gets 10 kb each side
        uint32_t nseq = 0; const char* const* names = nullptr; const uint64_t* lengths = nullptr;
        sp_fasta_sequences(h->fasta, &nseq, &names, &lengths);
        uint64_t clen = 0;
        for (uint32_t i = 0; i < nseq; ++i) if (h->cyp_chrom == names[i]) clen = lengths[i];
        ws = ws > 10000 ? ws - 10000 : 0; we = std::min(we + 10000, clen);
        const char* b = nullptr; uint64_t n = 0;
        if (sp_fasta_fetch(h->fasta, chrom, ws, we, &b, &n) != SP_OK) return fail(SP_ERR_INVALID_ARG, "CYP2D6: " + opt(sp_fasta_last_error(h->fasta)));
        const std::string window(b, n);
        sp_cyp_locus locus{}; sp_cyp_gene_def gd{}; sp_cyp_config cc{};
        if (sp_database_cyp_flatten(h->db, window.c_str(), ws, window.size(), &locus, &gd, &cc) != SP_OK)
            return fail(SP_ERR_INVALID_ARG, "CYP2D6: " + opt(sp_database_last_error(h->db)));
        const int32_t rc = sp_cyp_db_create(h->ctx2, &locus, &gd, &cc, &h->cyp);
        if (rc != SP_OK) return fail(rc, "sp_cyp_db_create: " + opt(sp_last_error(h->ctx2)));
        // extraction_region (src/cyp2d6/definitions.rs:72-99; STAR5_PRE_BUFFER 500, STAR5_POST_BUFFER 3000)
        h->cyp_start = std::min({locus.d6_start, locus.star5_start - 500, locus.d7_start, locus.rep6_start, locus.rep7_start});
        h->cyp_end = std::max({locus.d6_end, locus.star5_end + 3000, locus.d7_end, locus.rep6_end, locus.rep7_end});
        return SP_OK;
    };
    if (!settings->debug_skip_hla && setup_hla() != SP_OK) { h->hla_err = g_create_error; h->hgenes.clear(); g_create_error.clear(); }
    if (h->cyp_selected && setup_cyp() != SP_OK) { h->cyp_err = g_create_error; g_create_error.clear(); }
    *out = h.release();
    return SP_OK;
}

const char* sp_starphase_sample_error(const sp_starphase* h, uint32_t i) { return h && i < h->batch_err.size() ? h->batch_err[i].c_str() : ""; }
const char* sp_starphase_sample_warnings(const sp_starphase* h, uint32_t i) { return h && i < h->batch_warn.size() ? h->batch_warn[i].c_str() : ""; }
int32_t sp_starphase_last_batch_timing(const sp_starphase* h, sp_starphase_batch_timing* out) {
    if (!h || !out) return SP_ERR_INVALID_ARG;
    *out = h->batch_timing;
    return SP_OK;
}

int32_t sp_starphase_call_batch(sp_starphase* h, uint32_t n, const sp_sample_inputs* inputs, const char* const* debug_folders, const sp_batch_options* opts,
                                sp_result** out, int32_t* sample_rc) {
    if (!h) return SP_ERR_INVALID_ARG;
    h->err.clear(); h->warnings.clear(); h->batch_timing = sp_starphase_batch_timing{};
    if (n && (!inputs || !out)) return h->fail(SP_ERR_INVALID_ARG, "sp_starphase_call_batch: null argument");
    if (!h->debug_folder.empty() && !debug_folders)
        return h->fail(SP_ERR_INVALID_ARG, "sp_starphase_call_batch: the handle has a debug folder, which every sample would overwrite; pass debug_folders");
    const auto t_call = std::chrono::steady_clock::now();
    const uint32_t max_group = opts && opts->max_group ? opts->max_group : 64u;
    const uint32_t hw = std::max(1u, std::thread::hardware_concurrency());
    const uint32_t n_threads = opts && opts->decode_threads ? opts->decode_threads : std::min(16u, hw);
    h->batch_err.assign(n, std::string()); h->batch_warn.assign(n, std::string());
    for (uint32_t i = 0; i < n; ++i) { out[i] = nullptr; if (sample_rc) sample_rc[i] = SP_OK; }
    std::vector<Sample> S(n);
    for (uint32_t i = 0; i < n; ++i) sample_setup(h, inputs[i], debug_folders && debug_folders[i] ? std::string(debug_folders[i]) : std::string(), S[i]);
    sp_starphase_batch_timing& T = h->batch_timing;
    T.n_samples = n;
    // host decode of a group on the worker pool; group k + 1 is decoded while group k is on the device
    auto decode = [&](uint32_t g0, uint32_t g1, double* ms) {
        const auto t0 = std::chrono::steady_clock::now();
        std::atomic<uint32_t> next(g0);
        auto work = [&]() { for (uint32_t i; (i = next.fetch_add(1)) < g1;) decode_sample(h, S[i]); };
        std::vector<std::thread> pool;
        for (uint32_t t = 1; t < std::min(n_threads, g1 - g0); ++t) {
            try { pool.emplace_back(work); } catch (const std::system_error&) { break; }
        }
        work();
        for (auto& t : pool) t.join();
        *ms = ms_since(t0);
    };
    std::thread ahead; double ahead_ms = 0;
    int32_t first_rc = SP_OK;
    for (uint32_t g0 = 0; g0 < n; g0 += max_group) {
        const uint32_t g1 = std::min(n, g0 + max_group);
        if (g0 == 0) decode(g0, g1, &ahead_ms);
        else ahead.join();
        T.decode_ms += ahead_ms; ++T.n_groups;
        if (g1 < n) ahead = std::thread(decode, g1, std::min(n, g1 + max_group), &ahead_ms);
        std::vector<Sample*> group;
        for (uint32_t i = g0; i < g1; ++i) group.push_back(&S[i]);
        // CYP2D6 on its own thread and context, beside the variant genes and the HLA genes (settings.sequential: after them)
        double cyp_ms = 0;
        std::thread cyp;
        if (!h->s.sequential) cyp = std::thread(cyp_group, h, group, false, &cyp_ms);
        auto t0 = std::chrono::steady_clock::now();
        std::vector<VarSample*> vs;
        for (Sample* b : group) if (b->rc == SP_OK) { if (h->variant_alternatives) b->alt_folder = b->debug; vs.push_back(b); }
        variant_samples(h, vs);
        for (VarSample* v : vs) if (v->rc != SP_OK) static_cast<Sample*>(v)->stage = 1;
        T.variant_ms += ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        T.n_hla_reads += hla_group(h, group);
        T.hla_ms += ms_since(t0);
        if (cyp.joinable()) cyp.join();
        else cyp_group(h, group, true, &cyp_ms);
        T.cyp_ms += cyp_ms;
        t0 = std::chrono::steady_clock::now();
        for (uint32_t i = g0; i < g1; ++i) {
            Sample& b = S[i];
            if (b.run_cyp) T.n_cyp_reads += b.cyp.n_reads;
            sample_result(h, b, &out[i]);
            if (b.rc != SP_OK) { ++T.n_failed; if (first_rc == SP_OK) { first_rc = b.rc; h->err = "sample " + std::to_string(i) + ": " + b.err; } }
            if (sample_rc) sample_rc[i] = b.rc;
            h->batch_err[i] = b.err; h->batch_warn[i] = b.warnings;
        }
        T.package_ms += ms_since(t0);
    }
    T.wall_ms = ms_since(t_call);
    return first_rc;
}

// The pipeline for a group of one.  Nothing is decoded ahead: the CYP2D6 lane reads its BAM region on its own thread beside the variant genes and the
// HLA decode.  On a caller's context in exhaustive K1 mode (k1_best_n = 0) no read is named after a reverse-strand mapping (hla_pass).
int32_t sp_starphase_call(sp_starphase* h, const sp_sample_inputs* in, sp_result** out) {
    if (!h || !in || !out) return SP_ERR_INVALID_ARG;
    *out = nullptr;
    h->err.clear(); h->warnings.clear(); h->timing = sp_starphase_timing{};
    const auto t_call = std::chrono::steady_clock::now();
    Sample b;
    sample_setup(h, *in, h->debug_folder, b);
    if (b.rc != SP_OK) return h->fail(b.rc, b.err);
    const std::vector<Sample*> one{&b};
    sp_starphase_timing& T = h->timing;
    // the CYP2D6 lane: on its own host thread and context unless sequential
    std::thread worker;
    if (b.run_cyp && !h->s.sequential) worker = std::thread(cyp_group, h, one, false, &T.cyp_ms);
    auto t0 = std::chrono::steady_clock::now();
    if (b.has_vcf) {
        vcf_fetch(h, h->win, b.vcf, b.sv, b.sample, b.vf);
        if (h->variant_alternatives) b.alt_folder = b.debug;
        variant_samples(h, {&b});
        if (b.rc != SP_OK) b.stage = 1;
    }
    T.variant_ms = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    if (b.run_hla && b.rc == SP_OK) {
        hla_decode(h, b);
        T.bam_decode_ms = ms_since(t0);
        T.n_hla_reads = (uint32_t)hla_group(h, one);
    }
    T.hla_ms = ms_since(t0);
    if (worker.joinable()) worker.join();
    else if (b.run_cyp) cyp_group(h, one, true, &T.cyp_ms);
    T.bam_decode_ms += b.cyp.decode_ms; T.n_cyp_reads = b.cyp.n_reads;
    sample_result(h, b, out);
    h->warnings = b.warnings;
    if (b.rc != SP_OK) return h->fail(b.rc, b.err);
    T.call_ms = ms_since(t_call);
    return SP_OK;
}

}  // extern "C"

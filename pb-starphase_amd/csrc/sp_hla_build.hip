// sp_hla_build.hip -- update-hla: the HLA half of the reference's database build, without its downloads.
//
// Host: the two FASTA files of an IMGT/HLA release -> the allele table (convert_fasta_str_to_map + collapse_hla_lookup, src/build_database.rs:233-325;
// HlaAlleleDefinition::new, src/hla/alleles.rs:353-382).  Device: HlaConfig::new (src/hla/alleles.rs:109-207) -- every DNA allele of every gene mapped onto
// that gene's reference window +- 2,000 bases, the gene's coordinates stretched over each allele's best mapping.  The reference makes one minimap2 call per
// allele on one thread; here a gene's alleles are (allele, strand) cells of a batch: the k-mer vote anchor and the two-piece affine re-score (the pair that
// reports minimap2's numbers, sp_affine.hip) run back to back on the device, hlacfg_pick_extend_kernel picks per allele and reduces per gene.  The host sees
// one batch at a time, never an allele.
#include "sp_internal.h"
#include <algorithm>
#include <cctype>
#include <climits>
#include <cstring>
#include <memory>

int sp_seqset_build_index(sp_ctx* ctx, sp_seqset* s);                                           // sp_api.hip
bool spi_read_text_file(const char* path, std::string& out, std::string& err);                  // sp_database.hip: a file as it is, or inflated when it is gzip

struct sp_hla_alleles {
    struct Allele { std::string id, gene, star, dna, cdna; bool has_dna = false; };
    std::vector<Allele> alleles;                      // id order
    uint32_t n_dna = 0, dropped_no_cdna = 0, dropped_gene = 0;
    std::string warnings;
};

struct sp_hla_config_result {
    struct Gene { std::string name, chrom; uint64_t start = 0, end = 0; bool moved = false, absent = false;
                  int32_t worst_allele = -1, worst_len = 0, worst_nm = 0, worst_unm = 0; uint32_t n_dna = 0, n_mapped = 0; };
    std::vector<Gene> genes;                          // name order
    std::vector<sp_hla_cfg_mapping> maps;             // one per allele of the table
    std::string warnings;
};

namespace {

thread_local std::string g_fasta_err;

// SUPPORTED_HLA_GENES, ABSENT_HLA_GENES, HLA_COORDINATE_COPIES (src/hla/alleles.rs:16-70)
const char* const SUPPORTED[] = { "HLA-A", "HLA-B", "HLA-C", "HLA-DPA1", "HLA-DPB1", "HLA-DQA1", "HLA-DQB1", "HLA-DRB1", "HLA-DRB3", "HLA-DRB4", "HLA-DRB5" };
const char* const ABSENT[] = { "HLA-DRB3", "HLA-DRB4", "HLA-DRB5" };
const char* const COPIES[][2] = { { "HLA-DRB3", "HLA-DRB1" }, { "HLA-DRB4", "HLA-DRB1" } };      // (copy to, copy from)
bool is_supported(const std::string& g) { for (const char* s : SUPPORTED) if (g == s) return true; return false; }
bool is_absent_capable(const std::string& g) { for (const char* s : ABSENT) if (g == s) return true; return false; }

struct FastaRecord { std::string star, seq; };

// convert_fasta_str_to_map: bio::io::fasta records; id = the header's first word, description = the rest, star allele = the description's first word
bool fasta_to_map(const std::string& text, std::map<std::string, FastaRecord>& out, std::string& err) {
    size_t p = 0;
    std::string id; FastaRecord rec; bool open = false;
    auto close = [&]() -> bool {
        if (!open) return true;
        auto it = out.find(id);
        if (it == out.end()) out.emplace(id, rec);
        else if (it->second.star != rec.star || it->second.seq != rec.seq) { err = "FASTA record with multiple IDs/sequences detected: " + id; return false; }
        return true;
    };
    while (p < text.size()) {
        size_t e = text.find('\n', p);
        if (e == std::string::npos) e = text.size();
        size_t le = e;
        while (le > p && (text[le - 1] == '\r' || text[le - 1] == '\n')) --le;
        if (le > p && text[p] == '>') {
            if (!close()) return false;
            const std::string head = text.substr(p + 1, le - p - 1);
            const size_t sp = head.find(' ');
            id = head.substr(0, sp);
            rec = FastaRecord();
            if (sp != std::string::npos) {
                size_t a = sp;
                while (a < head.size() && std::isspace((unsigned char)head[a])) ++a;
                size_t b = a;
                while (b < head.size() && !std::isspace((unsigned char)head[b])) ++b;
                rec.star = head.substr(a, b - a);
            }
            open = true;
        } else if (le > p) {
            if (!open) { err = "Expected > at record start."; return false; }
            rec.seq.append(text, p, le - p);
        }
        p = e + 1;
    }
    return close();
}

bool all_acgt(const std::string& s) { for (char c : s) if (c != 'A' && c != 'C' && c != 'G' && c != 'T') return false; return true; }

int32_t fasta_fail(const std::string& m) { g_fasta_err = m; return SP_ERR_INVALID_ARG; }

// ---------------------------------------------------------------------------------------------------------------- the device side
// What a gene's alleles fold into: the extent of the chosen mappings on the window and the worst accepted score with its allele.  A score is the exact
// fraction num / (10 den): num = max(10 (nm + unmapped), 1) -- MappingScore::score_value's 0.1 for a perfect mapping --, den = the allele's length;
// num 0 = nothing.  Fractions are compared by cross-multiplication (num <= 2^21, den <= 2^17).
struct CfgFold { int32_t t_min, t_max; uint32_t w_num, w_den; int32_t w_idx, w_nm, w_unm, pad; };

__host__ __device__ inline CfgFold cfg_identity() { CfgFold f; f.t_min = INT_MAX; f.t_max = INT_MIN; f.w_num = 0; f.w_den = 1; f.w_idx = INT_MAX; f.w_nm = 0; f.w_unm = 0; f.pad = 0; return f; }

// the worse of the two scores; equal scores: the lower index (the reference walks the alleles in id order and replaces on strictly greater)
__device__ __forceinline__ CfgFold cfg_merge(const CfgFold& a, const CfgFold& b) {
    CfgFold r = a;
    r.t_min = b.t_min < a.t_min ? b.t_min : a.t_min;
    r.t_max = b.t_max > a.t_max ? b.t_max : a.t_max;
    bool take_b = false;
    if (b.w_num != 0) {
        if (a.w_num == 0) take_b = true;
        else {
            const unsigned long long l = (unsigned long long)b.w_num * a.w_den, r2 = (unsigned long long)a.w_num * b.w_den;
            take_b = l > r2 || (l == r2 && b.w_idx < a.w_idx);
        }
    }
    if (take_b) { r.w_num = b.w_num; r.w_den = b.w_den; r.w_idx = b.w_idx; r.w_nm = b.w_nm; r.w_unm = b.w_unm; }
    return r;
}

// a DPP move of the whole record; a lane the pattern gives no source keeps its own value, which the merge leaves as it is
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ CfgFold cfg_dpp(const CfgFold& v) {
    CfgFold r;
    r.t_min = __builtin_amdgcn_update_dpp(v.t_min, v.t_min, CTRL, ROW_MASK, 0xf, false);
    r.t_max = __builtin_amdgcn_update_dpp(v.t_max, v.t_max, CTRL, ROW_MASK, 0xf, false);
    r.w_num = (uint32_t)__builtin_amdgcn_update_dpp((int)v.w_num, (int)v.w_num, CTRL, ROW_MASK, 0xf, false);
    r.w_den = (uint32_t)__builtin_amdgcn_update_dpp((int)v.w_den, (int)v.w_den, CTRL, ROW_MASK, 0xf, false);
    r.w_idx = __builtin_amdgcn_update_dpp(v.w_idx, v.w_idx, CTRL, ROW_MASK, 0xf, false);
    r.w_nm = __builtin_amdgcn_update_dpp(v.w_nm, v.w_nm, CTRL, ROW_MASK, 0xf, false);
    r.w_unm = __builtin_amdgcn_update_dpp(v.w_unm, v.w_unm, CTRL, ROW_MASK, 0xf, false);
    r.pad = 0;
    return r;
}
// the fold of the 64 lanes arrives in lane 63 (the gfx9 reduction: row_shr 1, 2, 4, 8, then row_bcast 15 and 31); all 64 lanes call it
__device__ __forceinline__ CfgFold cfg_wave_fold(CfgFold v) {
    v = cfg_merge(v, cfg_dpp<0x111, 0xf>(v));
    v = cfg_merge(v, cfg_dpp<0x112, 0xf>(v));
    v = cfg_merge(v, cfg_dpp<0x114, 0xf>(v));
    v = cfg_merge(v, cfg_dpp<0x118, 0xf>(v));
    v = cfg_merge(v, cfg_dpp<0x142, 0xa>(v));
    v = cfg_merge(v, cfg_dpp<0x143, 0xc>(v));
    return v;
}

// cell x of a batch = sequence x of the batch's query set: allele x >> 1 of the batch, forward (x & 1 = 0) or reverse-complemented; one target, the window
__global__ void hlacfg_cells_kernel(uint32_t n_cells, uint32_t* __restrict__ a_idx, uint32_t* __restrict__ b_idx) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_cells) return;
    a_idx[x] = x; b_idx[x] = 0u;
}
// the re-score's pair list from the anchors; a cell without a vote is marked "skip" (score 0)
__global__ void hlacfg_pairs_kernel(uint32_t n_cells, const int32_t* __restrict__ diag, const int32_t* __restrict__ votes, sp_pair* __restrict__ pairs) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_cells) return;
    sp_pair p; p.a = x; p.b = 0u; p.diag = diag[x]; p.max_ed = votes[x] > 0 ? 0 : -1;
    pairs[x] = p;
}

constexpr int CFG_BAND = 256;
constexpr int CFG_MIN_DP_MAX = 200;       // mm_filter_regs with map-hifi's min_dp_max: minimap2 returns no mapping whose peak DP score is below it (a stray 16-mer vote re-scores to a 16-base match)
constexpr int CFG_THREADS = 256;

// One thread per allele of the batch: HlaConfig::new's choice among the allele's mappings (its two strands), its record, and the wave's fold
// into partial[wave of the grid].  first = position of the batch's first allele in the gene's list (the "index" of the tie rule).
__global__ __launch_bounds__(CFG_THREADS) void hlacfg_pick_extend_kernel(const sp_affine_aln* __restrict__ aff, const sp_pair* __restrict__ pairs, const int32_t* __restrict__ qlen,
                                                                        uint32_t n_alleles, uint32_t first, int32_t gene, sp_hla_cfg_mapping* __restrict__ rec,
                                                                        CfgFold* __restrict__ partial) {
    const uint32_t x = blockIdx.x * CFG_THREADS + threadIdx.x;
    CfgFold f = cfg_identity();
    if (x < n_alleles) {
        const int len = qlen[2 * x];
        sp_affine_aln m[2]; bool valid[2], edge[2];
        for (int c = 0; c < 2; ++c) {
            m[c] = aff[2 * x + c];
            const sp_pair p = pairs[2 * x + c];
            valid[c] = p.max_ed >= 0 && m[c].score >= CFG_MIN_DP_MAX;
            // diagonal of the first and of the last cell relative to the anchor: the band holds -128 .. 127
            const int k0 = m[c].a_start - m[c].b_start + p.diag, k1 = m[c].a_end - m[c].b_end + p.diag;
            edge[c] = valid[c] && (k0 <= -CFG_BAND / 2 || k0 >= CFG_BAND / 2 - 1 || k1 <= -CFG_BAND / 2 || k1 >= CFG_BAND / 2 - 1);
        }
        // minimap2's output order: the higher DP score first; the forward strand first on a tie
        const int order0 = (valid[1] && (!valid[0] || m[1].score > m[0].score)) ? 1 : 0;
        int pick = -1; uint32_t best_num = 10u * (uint32_t)len;                 // MappingStats::new(len, len, 0): score 1.0
        int best_nm = 0, best_unm = 0;
        for (int k = 0; k < 2; ++k) {
            const int c = k == 0 ? order0 : 1 - order0;
            if (!valid[c]) continue;
            const int unm = len - (m[c].a_end - m[c].a_start);
            const uint32_t num = (uint32_t)max(10 * (m[c].nm + unm), 1);
            if (num < best_num) { best_num = num; pick = c; best_nm = m[c].nm; best_unm = unm; }
        }
        sp_hla_cfg_mapping r; r.status = 0; r.rev = 0; r.nm = 0; r.q_start = r.q_end = r.t_start = r.t_end = 0; r.gene = gene;
        const bool overflow = pick >= 0 ? edge[pick] : (edge[0] || edge[1]);
        if (len <= 0 || overflow) r.status = -1;
        else if (pick >= 0) {
            r.status = 1; r.rev = pick; r.nm = best_nm;
            r.q_start = pick ? len - m[pick].a_end : m[pick].a_start; r.q_end = pick ? len - m[pick].a_start : m[pick].a_end;
            r.t_start = m[pick].b_start; r.t_end = m[pick].b_end;
            f.t_min = r.t_start; f.t_max = r.t_end;
            f.w_num = best_num; f.w_den = (uint32_t)len; f.w_idx = (int32_t)(first + x); f.w_nm = best_nm; f.w_unm = best_unm;
        }
        rec[x] = r;
    }
    f = cfg_wave_fold(f);
    if ((threadIdx.x & 63) == 63) partial[blockIdx.x * (CFG_THREADS / 64) + (threadIdx.x >> 6)] = f;
}

// the second pass: one wave folds the batch's partials into the gene's slot
__global__ __launch_bounds__(64) void hlacfg_fold_kernel(const CfgFold* __restrict__ partial, uint32_t n_partial, CfgFold* __restrict__ slot) {
    CfgFold f = cfg_identity();
    for (uint32_t i = threadIdx.x; i < n_partial; i += 64) f = cfg_merge(f, partial[i]);
    f = cfg_wave_fold(f);
    if (threadIdx.x == 63) *slot = cfg_merge(*slot, f);
}

char comp(char c) { switch (c) { case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A'; default: return 'N'; } }

struct StartGene { std::string name, chrom; uint64_t start, end; };

} // namespace

extern "C" {

const char* sp_hla_fasta_last_error(void) { return g_fasta_err.c_str(); }

int32_t sp_hla_fasta_load(const char* hla_gen, const char* hla_nuc, sp_hla_alleles** out) {
    if (!out) return fasta_fail("sp_hla_fasta_load: out is NULL");
    *out = nullptr;
    if (!hla_gen || !hla_nuc) return fasta_fail("sp_hla_fasta_load: a path is NULL");
    std::string text, err;
    std::map<std::string, FastaRecord> dna, cdna;
    if (!spi_read_text_file(hla_gen, text, err)) return fasta_fail(err);
    if (!fasta_to_map(text, dna, err)) return fasta_fail(err);
    text.clear();
    if (!spi_read_text_file(hla_nuc, text, err)) return fasta_fail(err);
    if (!fasta_to_map(text, cdna, err)) return fasta_fail(err);
    auto tab = std::make_unique<sp_hla_alleles>();
    // collapse_hla_lookup: every DNA has a cDNA, but not all cDNAs have a DNA
    for (const auto& kv : dna) if (!cdna.count(kv.first)) ++tab->dropped_no_cdna;
    if (tab->dropped_no_cdna) tab->warnings += "Detected " + std::to_string(tab->dropped_no_cdna) + " DNA entries that do not have a cDNA, ignoring them.\n";
    for (const auto& kv : cdna) {                                  // (std::map: id order, the BTreeMap's)
        sp_hla_alleles::Allele a; a.id = kv.first; a.cdna = kv.second.seq;
        const std::string& desc = kv.second.star;
        auto d = dna.find(kv.first);
        if (d != dna.end()) {
            if (d->second.star != desc) return fasta_fail(kv.first + " has description \"" + d->second.star + "\" for DNA and \"" + desc + "\" for cDNA.");
            a.has_dna = true; a.dna = d->second.seq;
        }
        // HlaAlleleDefinition::new
        const size_t star = desc.find('*');
        if (star == std::string::npos || desc.find('*', star + 1) != std::string::npos) return fasta_fail("Star split length != 2 for allele description: " + desc);
        a.gene = "HLA-" + desc.substr(0, star);
        a.star = desc.substr(star + 1);
        if (std::count(a.star.begin(), a.star.end(), ':') > 3) return fasta_fail("Unexpected number of fields for allele description: " + desc);
        if (a.has_dna && !all_acgt(a.dna)) return fasta_fail("DNA sequence contains non-ACGT symbols.");
        if (!all_acgt(a.cdna)) return fasta_fail("cDNA sequence contains non-ACGT symbols.");
        if (!is_supported(a.gene)) { ++tab->dropped_gene; continue; }
        if (a.has_dna) ++tab->n_dna;
        tab->alleles.push_back(std::move(a));
    }
    if (tab->dropped_gene) tab->warnings += "Removed " + std::to_string(tab->dropped_gene) + " alleles that are not in supported HLA gene set.\n";
    *out = tab.release();
    return SP_OK;
}

void sp_hla_alleles_free(sp_hla_alleles* alleles) { delete alleles; }

int32_t sp_hla_alleles_info(const sp_hla_alleles* t, sp_hla_alleles_stats* out) {
    if (!t || !out) return SP_ERR_INVALID_ARG;
    *out = sp_hla_alleles_stats{ (uint32_t)t->alleles.size(), t->n_dna, t->dropped_no_cdna, t->dropped_gene, t->warnings.c_str() };
    return SP_OK;
}

int32_t sp_hla_alleles_get(const sp_hla_alleles* t, uint32_t i, const char** hla_id, const char** gene_name, const char** star_allele, const char** dna, const char** cdna) {
    if (!t || i >= t->alleles.size()) return SP_ERR_INVALID_ARG;
    const auto& a = t->alleles[i];
    if (hla_id) *hla_id = a.id.c_str();
    if (gene_name) *gene_name = a.gene.c_str();
    if (star_allele) *star_allele = a.star.c_str();
    if (dna) *dna = a.has_dna ? a.dna.c_str() : nullptr;
    if (cdna) *cdna = a.cdna.c_str();
    return SP_OK;
}

int32_t sp_hla_config_result_create(uint32_t n_genes, const char* const* names, const uint64_t* start, const uint64_t* end, sp_hla_config_result** out) {
    if (!out || (n_genes && (!names || !start || !end))) return SP_ERR_INVALID_ARG;
    *out = nullptr;
    auto r = std::make_unique<sp_hla_config_result>();
    for (uint32_t g = 0; g < n_genes; ++g) {
        if (!names[g] || start[g] > end[g]) return SP_ERR_INVALID_ARG;
        sp_hla_config_result::Gene x; x.name = names[g]; x.start = start[g]; x.end = end[g]; x.absent = is_absent_capable(x.name);
        r->genes.push_back(std::move(x));
    }
    std::sort(r->genes.begin(), r->genes.end(), [](const auto& a, const auto& b) { return a.name < b.name; });
    *out = r.release();
    return SP_OK;
}

void sp_hla_config_result_free(sp_hla_config_result* result) { delete result; }

int32_t sp_hla_config_result_info(const sp_hla_config_result* r, uint32_t* n_genes, uint32_t* n_alleles, const char** warnings) {
    if (!r) return SP_ERR_INVALID_ARG;
    if (n_genes) *n_genes = (uint32_t)r->genes.size();
    if (n_alleles) *n_alleles = (uint32_t)r->maps.size();
    if (warnings) *warnings = r->warnings.c_str();
    return SP_OK;
}

int32_t sp_hla_config_result_gene(const sp_hla_config_result* r, uint32_t g, sp_hla_cfg_gene* out) {
    if (!r || !out || g >= r->genes.size()) return SP_ERR_INVALID_ARG;
    const auto& x = r->genes[g];
    *out = sp_hla_cfg_gene{ x.name.c_str(), x.chrom.c_str(), x.start, x.end, x.moved ? 1 : 0, x.absent ? 1 : 0, x.worst_allele, x.worst_len, x.worst_nm, x.worst_unm, x.n_dna, x.n_mapped };
    return SP_OK;
}

int32_t sp_hla_config_result_mapping(const sp_hla_config_result* r, uint32_t allele, sp_hla_cfg_mapping* out) {
    if (!r || !out || allele >= r->maps.size()) return SP_ERR_INVALID_ARG;
    *out = r->maps[allele];
    return SP_OK;
}

int32_t sp_hla_config_extend(sp_ctx* ctx, sp_fasta* reference, const sp_database* db, const sp_hla_alleles* alleles, uint32_t batch_alleles, sp_hla_config_result** out) {
    if (!ctx) return SP_ERR_INVALID_ARG;
    if (!reference || !alleles || !out) return sp_fail(ctx, SP_ERR_INVALID_ARG, "hla_config_extend: reference, alleles and out are required");
    *out = nullptr;
    (void)hipSetDevice(ctx->device);
    if (batch_alleles == 0) batch_alleles = 1024;
    constexpr uint64_t BATCH_BASES = 16ull << 20;                 // allele bases per pass (both strands are uploaded: twice this)
    constexpr uint64_t BUFFER = 2000;
    // the starting collection: the database's hla_config (the two-gene default when it has none), SUPPORTED_HLA_GENES only, then copy_missing_genes
    sp_database* own_db = nullptr;
    if (!db) {
        static const char EMPTY_DB[] = "{\"database_metadata\":{\"pbstarphase_version\":\"\",\"cpic_version\":\"\",\"hla_version\":\"\",\"pharmvar_version\":\"\",\"build_time\":\"\"}}";
        char err[256];
        if (sp_database_parse(EMPTY_DB, sizeof EMPTY_DB - 1, &own_db, err, sizeof err) != SP_OK) return sp_fail(ctx, SP_ERR_INVALID_ARG, std::string("hla_config_extend: ") + err);
        db = own_db;
    }
    std::vector<StartGene> start_genes;
    {
        sp_database_stats st{};
        sp_database_info(db, &st);
        for (uint32_t g = 0; g < st.n_hla_genes; ++g) {
            sp_gene_region r{};
            sp_database_hla_gene(db, g, &r);
            if (is_supported(r.name)) start_genes.push_back(StartGene{ r.name, r.chrom, r.start, r.end });
        }
        for (const auto& cp : COPIES) {
            const StartGene* from = nullptr; bool have = false;
            for (const StartGene& s : start_genes) { if (s.name == cp[1]) from = &s; if (s.name == cp[0]) have = true; }
            if (from && !have) { StartGene c = *from; c.name = cp[0]; start_genes.push_back(c); }
        }
        std::sort(start_genes.begin(), start_genes.end(), [](const StartGene& a, const StartGene& b) { return a.name < b.name; });
    }
    if (own_db) sp_database_free(own_db);
    uint32_t n_chrom = 0; const char* const* chrom_names = nullptr; const uint64_t* chrom_len = nullptr;
    if (sp_fasta_sequences(reference, &n_chrom, &chrom_names, &chrom_len) != SP_OK) return sp_fail(ctx, SP_ERR_INVALID_ARG, std::string("hla_config_extend: ") + sp_fasta_last_error(reference));

    auto res = std::make_unique<sp_hla_config_result>();
    const auto& tab = alleles->alleles;
    sp_hla_cfg_mapping none{}; none.gene = -1;
    res->maps.assign(tab.size(), none);
    const size_t n_genes = start_genes.size();
    CfgFold* d_slots = (CfgFold*)sp_pool(ctx, "hlacfg_slots", std::max<size_t>(1, n_genes) * sizeof(CfgFold));
    if (!d_slots) return sp_fail(ctx, SP_ERR_OUT_OF_MEMORY, "hla_config_extend: gene slots");
    std::vector<CfgFold> slots(n_genes, cfg_identity());
    std::vector<std::vector<uint32_t>> lists(n_genes);              // per gene: its alleles with DNA, id order
    for (size_t g = 0; g < n_genes; ++g) {
        const StartGene& sg = start_genes[g];
        if (sg.start < BUFFER)
            return sp_fail(ctx, SP_ERR_INVALID_ARG, "hla_config_extend: the alignment window of " + sg.name + " starts before " + sg.chrom + " (gene start " + std::to_string(sg.start) + " < 2000)");
        uint64_t clen = 0; bool found = false;
        for (uint32_t c = 0; c < n_chrom; ++c) if (sg.chrom == chrom_names[c]) { clen = chrom_len[c]; found = true; }
        if (!found) return sp_fail(ctx, SP_ERR_INVALID_ARG, "hla_config_extend: the reference has no sequence " + sg.chrom + " (" + sg.name + ")");
        if (sg.end + BUFFER > clen) return sp_fail(ctx, SP_ERR_INVALID_ARG, "hla_config_extend: the alignment window of " + sg.name + " ends behind " + sg.chrom);
        // worst starts as the perfect match of the window: MappingStats::new(ref_len, 0, 0)
        slots[g].w_num = 1; slots[g].w_den = (uint32_t)(sg.end - sg.start + 2 * BUFFER); slots[g].w_idx = -1;
        for (size_t i = 0; i < tab.size(); ++i) if (tab[i].gene == sg.name) { res->maps[i].gene = (int32_t)g; if (tab[i].has_dna) lists[g].push_back((uint32_t)i); }
    }
    if (n_genes) SP_HIP_CHECK(ctx, hipMemcpyAsync(d_slots, slots.data(), n_genes * sizeof(CfgFold), hipMemcpyHostToDevice, ctx->stream));
    SP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));           // (slots is a local: the copy has to be over before it can go)
    const sp_affine_opts opts{ 1, 4, 6, 2, 26, 1, 1 };
    std::vector<sp_hla_cfg_mapping> batch_rec;
    for (size_t g = 0; g < n_genes; ++g) {
        const StartGene& sg = start_genes[g];
        const std::vector<uint32_t>& list = lists[g];
        if (list.empty()) continue;
        const char* win = nullptr; uint64_t win_len = 0;
        if (sp_fasta_fetch(reference, sg.chrom.c_str(), sg.start - BUFFER, sg.end + BUFFER, &win, &win_len) != SP_OK)
            return sp_fail(ctx, SP_ERR_INVALID_ARG, std::string("hla_config_extend: ") + sp_fasta_last_error(reference));
        const uint64_t t_off[2] = { 0, win_len };
        sp_seqset* T = nullptr;
        int32_t rc = sp_seqset_upload(ctx, win, t_off, 1, &T);
        if (rc != SP_OK) return rc;
        uint32_t t_skipped = 0; sp_seqset_skipped(T, &t_skipped);
        if (t_skipped) { sp_seqset_free(T); return sp_fail(ctx, SP_ERR_TOO_LONG, "hla_config_extend: the window of " + sg.name + " is longer than 65,534 bases"); }
        for (size_t first = 0; first < list.size() && rc == SP_OK;) {
            size_t n = 0; uint64_t bases = 0;
            while (first + n < list.size() && n < batch_alleles && (n == 0 || bases + tab[list[first + n]].dna.size() <= BATCH_BASES)) { bases += tab[list[first + n]].dna.size(); ++n; }
            // the batch's query set: every allele as given and reverse-complemented
            std::string q; q.reserve(2 * bases);
            std::vector<uint64_t> q_off(2 * n + 1, 0);
            for (size_t x = 0; x < n; ++x) {
                const std::string& s = tab[list[first + x]].dna;
                q += s; q_off[2 * x + 1] = q.size();
                for (size_t k = s.size(); k-- > 0;) q += comp(s[k]);
                q_off[2 * x + 2] = q.size();
            }
            sp_seqset* Q = nullptr;
            rc = sp_seqset_upload(ctx, q.data(), q_off.data(), (uint32_t)(2 * n), &Q);
            if (rc != SP_OK) break;
            const uint32_t n_cells = (uint32_t)(2 * n), n_partial = (uint32_t)((n + CFG_THREADS - 1) / CFG_THREADS) * (CFG_THREADS / 64);
            rc = sp_seqset_build_index(ctx, Q);
            uint32_t* d_a = (uint32_t*)sp_pool(ctx, "hlacfg_a", (size_t)n_cells * 4); uint32_t* d_b = (uint32_t*)sp_pool(ctx, "hlacfg_b", (size_t)n_cells * 4);
            int32_t* d_diag = (int32_t*)sp_pool(ctx, "hlacfg_diag", (size_t)n_cells * 4); int32_t* d_votes = (int32_t*)sp_pool(ctx, "hlacfg_votes", (size_t)n_cells * 4);
            sp_pair* d_pairs = (sp_pair*)sp_pool(ctx, "hlacfg_pairs", (size_t)n_cells * sizeof(sp_pair));
            sp_affine_aln* d_aff = (sp_affine_aln*)sp_pool(ctx, "hlacfg_aff", (size_t)n_cells * sizeof(sp_affine_aln));
            sp_hla_cfg_mapping* d_rec = (sp_hla_cfg_mapping*)sp_pool(ctx, "hlacfg_rec", n * sizeof(sp_hla_cfg_mapping));
            CfgFold* d_partial = (CfgFold*)sp_pool(ctx, "hlacfg_partial", (size_t)n_partial * sizeof(CfgFold));
            if (rc == SP_OK && !(d_a && d_b && d_diag && d_votes && d_pairs && d_aff && d_rec && d_partial)) rc = sp_fail(ctx, SP_ERR_OUT_OF_MEMORY, "hla_config_extend: batch buffers");
            if (rc == SP_OK) {
                const unsigned cell_blocks = (n_cells + 255) / 256;
                hipLaunchKernelGGL(hlacfg_cells_kernel, dim3(cell_blocks), dim3(256), 0, ctx->stream, n_cells, d_a, d_b);
                rc = sp_launch_anchor(ctx, Q, T, d_a, d_b, n_cells, d_diag, d_votes, 1, "hlacfg_anchor");
                if (rc == SP_OK) {
                    hipLaunchKernelGGL(hlacfg_pairs_kernel, dim3(cell_blocks), dim3(256), 0, ctx->stream, n_cells, d_diag, d_votes, d_pairs);
                    rc = sp_launch_affine(ctx, Q, T, d_pairs, n_cells, opts, CFG_BAND, d_aff, "hlacfg_affine");
                }
                if (rc == SP_OK) {
                    ProfScope ps(ctx, "hlacfg_pick_extend", n);
                    hipLaunchKernelGGL(hlacfg_pick_extend_kernel, dim3((unsigned)((n + CFG_THREADS - 1) / CFG_THREADS)), dim3(CFG_THREADS), 0, ctx->stream,
                                       d_aff, d_pairs, Q->d_len, (uint32_t)n, (uint32_t)first, (int32_t)g, d_rec, d_partial);
                    hipLaunchKernelGGL(hlacfg_fold_kernel, dim3(1), dim3(64), 0, ctx->stream, d_partial, n_partial, d_slots + g);
                    if (hipGetLastError() != hipSuccess) rc = sp_fail(ctx, SP_ERR_HIP, "hla_config_extend: launch failed");
                }
                if (rc == SP_OK) {
                    batch_rec.resize(n);
                    if (hipMemcpyAsync(batch_rec.data(), d_rec, n * sizeof(sp_hla_cfg_mapping), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                        hipStreamSynchronize(ctx->stream) != hipSuccess) rc = sp_fail(ctx, SP_ERR_HIP, std::string("hla_config_extend: ") + hipGetErrorString(hipGetLastError()));
                }
            }
            sp_seqset_free(Q);                                      // (waits for the stream: the one synchronisation of the batch)
            if (rc != SP_OK) break;
            for (size_t x = 0; x < n; ++x) {
                const uint32_t a = list[first + x];
                res->maps[a] = batch_rec[x];
                if (batch_rec[x].status < 0)
                    res->warnings += tab[a].id + " (" + tab[a].gene + "*" + tab[a].star + "): " + (tab[a].dna.size() > 65534 ? "longer than 65,534 bases" : "the re-score reached the edge of its band") + ", no mapping is reported\n";
            }
            first += n;
        }
        sp_seqset_free(T);
        if (rc != SP_OK) return rc;
    }
    if (n_genes) {
        SP_HIP_CHECK(ctx, hipMemcpyAsync(slots.data(), d_slots, n_genes * sizeof(CfgFold), hipMemcpyDeviceToHost, ctx->stream));
        SP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    }
    for (size_t g = 0; g < n_genes; ++g) {
        const StartGene& sg = start_genes[g];
        sp_hla_config_result::Gene x; x.name = sg.name; x.chrom = sg.chrom; x.start = sg.start; x.end = sg.end; x.absent = is_absent_capable(sg.name);
        x.n_dna = (uint32_t)lists[g].size();
        for (uint32_t a : lists[g]) if (res->maps[a].status == 1) ++x.n_mapped;
        const CfgFold& f = slots[g];
        if (f.t_min != INT_MAX) {                                   // extend_coordinates over every chosen mapping at once: min / max are what the loop leaves
            const uint64_t lo = sg.start - BUFFER + (uint64_t)f.t_min, hi = sg.start - BUFFER + (uint64_t)f.t_max;
            if (lo < x.start) { x.start = lo; x.moved = true; }
            if (hi > x.end) { x.end = hi; x.moved = true; }
        }
        if (f.w_idx >= 0 && (size_t)f.w_idx < lists[g].size()) { x.worst_allele = (int32_t)lists[g][(size_t)f.w_idx]; x.worst_len = (int32_t)f.w_den; x.worst_nm = f.w_nm; x.worst_unm = f.w_unm; }
        res->genes.push_back(std::move(x));
    }
    *out = res.release();
    return SP_OK;
}

} // extern "C"

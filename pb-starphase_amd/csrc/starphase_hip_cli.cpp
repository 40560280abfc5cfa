// starphase_hip_cli.cpp -- `starphase_hip diplotype ...`: the reference's `pbstarphase diplotype` command (src/main.rs, src/cli/diplotype.rs) on
// libstarphase_hip.  Flag names and defaults are the reference's for everything sp_starphase_call supports; exit codes as the reference's:
// 2 for a command line that does not parse (clap), NOINPUT (66) for an input file that does not exist, USAGE (64) when check_diplotype_settings
// refuses the settings, IOERR (74) for the database / reference / output files, DATAERR (65) when the call fails.  Every check of the command
// line is made before the first device call.  `starphase_hip diplotype-batch` types the samples of a manifest through sp_starphase_call_batch.
#include "../../include/starphase_hip.h"
#include <sys/stat.h>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

enum { EX_OK_ = 0, EX_CLAP = 2, EX_USAGE_ = 64, EX_DATAERR_ = 65, EX_NOINPUT_ = 66, EX_UNAVAILABLE_ = 69, EX_IOERR_ = 74 };

const char* HELP =
    "Diplotype a sample from its VCF / BAM files against a PGx database (pbstarphase diplotype)\n"
    "\n"
    "Usage: starphase_hip diplotype [OPTIONS] --database <JSON> --reference <FASTA> --output-calls <JSON>\n"
    "\n"
    "Input/Output:\n"
    "  -d, --database <JSON>            Input database file (JSON)\n"
    "  -r, --reference <FASTA>          Reference FASTA file\n"
    "  -c, --vcf <VCF>                  Input variant file in VCF format\n"
    "  -s, --sv-vcf <VCF>               Input structural variant file in VCF format\n"
    "  -b, --bam <BAM>                  Input alignment file in BAM format, can be specified multiple times; required for HLA diplotyping\n"
    "  -o, --output-calls <JSON>        Output diplotype call file (JSON)\n"
    "      --pharmcat-tsv <TSV>         Output file that can be provided to PharmCAT for further call interpretation\n"
    "      --include-set <TXT>          Optional file indicating the list of genes to include in diplotyping, one per line\n"
    "      --exclude-set <TXT>          Optional file indicating the list of genes to exclude from diplotyping, one per line\n"
    "      --output-debug <DIR>         Optional output debug folder (hla_debug.json, cyp2d6_alleles.json)\n"
    "      --debug-reads                Also write read_debug.json there: every realigned HLA read's accepted allele with CIGAR and MD (needs --output-debug)\n"
    "      --sample-name <STRING>       Sample name from the input VCFs (default: first sample)\n"
    "\n"
    "Variant parameters:\n"
    "      --max-sv-length <BASEPAIRS>  The maximum length of an SV to consider, anything longer is ignored [default: 1000000]\n"
    "\n"
    "HLA calling:\n"
    "      --disable-cdna-scoring       Disables scoring by cDNA (implies --hla-require-dna)\n"
    "      --hla-require-dna            Requires HLA alleles to have a DNA sequence definition\n"
    "      --max-error-rate <FLOAT>     The maximum error rate for a read to the HLA reference allele [default: 0.07]\n"
    "      --min-cdf-prob <FLOAT>       The minimum cumulative distribution function probability for a heterozygous call [default: 0.001]\n"
    "      --expected-maf <FLOAT>       Expected minor allele frequency; reduce to account for skew from sequencing bias [default: 0.45]\n"
    "      --debug-skip-hla             Skips HLA diplotyping\n"
    "\n"
    "CYP2D6 calling:\n"
    "      --infer-connections          Enables inferrence of connected alleles based on population observations\n"
    "      --normalize-d6-only          Disables normalizing coverage with D7 and hybrid alleles\n"
    "\n"
    "Consensus (HLA and CYP2D6):\n"
    "      --min-consensus-fraction <FLOAT>  The minimum fraction of sequences required to split into multiple consensuses (e.g. MAF) [default: 0.10]\n"
    "      --min-consensus-count <COUNT>     The minimum counts of sequences required to split into multiple consensuses [default: 3]\n"
    "      --dual-max-ed-delta <COUNT>       The edit distance delta threshold to stop tracking divergent sequences (efficiency heuristic) [default: 100]\n"
    "\n"
    "Execution:\n"
    "      --sequential                 Run the variant genes, the HLA genes and CYP2D6 one after another (the calls are the same)\n"
    "  -t, --threads <THREADS>          Accepted for compatibility; the reference deprecates it [default: 1]\n"
    "  -v, --verbose...                 Enable verbose output (print the warnings and timings of the call)\n"
    "  -h, --help                       Print help\n"
    "\n"
    "Not supported here: --hla-revert-method, --output-cyp2d6-bam, --debug-hla-target\n";

bool exists(const std::string& p) { struct stat st; return ::stat(p.c_str(), &st) == 0; }

int clap_error(const std::string& m) {
    std::fprintf(stderr, "error: %s\n\nUsage: starphase_hip diplotype [OPTIONS] --database <JSON> --reference <FASTA> --output-calls <JSON>\n\nFor more information, try '--help'.\n", m.c_str());
    return EX_CLAP;
}

bool parse_f64(const std::string& s, double* out) { char* end = nullptr; errno = 0; *out = std::strtod(s.c_str(), &end); return !s.empty() && end && *end == 0 && errno == 0; }
bool parse_u64(const std::string& s, uint64_t* out) {
    if (s.empty() || s[0] == '-' || s[0] == '+') return false;
    char* end = nullptr; errno = 0; *out = std::strtoull(s.c_str(), &end, 10); return end && *end == 0 && errno == 0;
}

const char* BATCH_HELP =
    "Diplotype many samples, listed in a manifest, against one PGx database (many samples per device pass)\n"
    "\n"
    "Usage: starphase_hip diplotype-batch [OPTIONS] --database <JSON> --reference <FASTA> --manifest <TSV>\n"
    "\n"
    "Input/Output:\n"
    "  -d, --database <JSON>            Input database file (JSON)\n"
    "  -r, --reference <FASTA>          Reference FASTA file\n"
    "  -m, --manifest <TSV>             One sample per line, tab-separated: output_calls, bams (comma-separated), vcf, sample_name, sv_vcf,\n"
    "                                   pharmcat_tsv, output_debug ('-' or empty = none); lines starting with '#' are headers\n"
    "      --include-set <TXT>          Optional file indicating the list of genes to include in diplotyping, one per line\n"
    "      --exclude-set <TXT>          Optional file indicating the list of genes to exclude from diplotyping, one per line\n"
    "\n"
    "Variant parameters:\n"
    "      --max-sv-length <BASEPAIRS>  The maximum length of an SV to consider, anything longer is ignored [default: 1000000]\n"
    "\n"
    "HLA calling:\n"
    "      --disable-cdna-scoring       Disables scoring by cDNA (implies --hla-require-dna)\n"
    "      --hla-require-dna            Requires HLA alleles to have a DNA sequence definition\n"
    "      --max-error-rate <FLOAT>     The maximum error rate for a read to the HLA reference allele [default: 0.07]\n"
    "      --min-cdf-prob <FLOAT>       The minimum cumulative distribution function probability for a heterozygous call [default: 0.001]\n"
    "      --expected-maf <FLOAT>       Expected minor allele frequency; reduce to account for skew from sequencing bias [default: 0.45]\n"
    "      --debug-skip-hla             Skips HLA diplotyping\n"
    "\n"
    "CYP2D6 calling:\n"
    "      --infer-connections          Enables inferrence of connected alleles based on population observations\n"
    "      --normalize-d6-only          Disables normalizing coverage with D7 and hybrid alleles\n"
    "\n"
    "Consensus (HLA and CYP2D6):\n"
    "      --min-consensus-fraction <FLOAT>  The minimum fraction of sequences required to split into multiple consensuses (e.g. MAF) [default: 0.10]\n"
    "      --min-consensus-count <COUNT>     The minimum counts of sequences required to split into multiple consensuses [default: 3]\n"
    "      --dual-max-ed-delta <COUNT>       The edit distance delta threshold to stop tracking divergent sequences (efficiency heuristic) [default: 100]\n"
    "\n"
    "Execution:\n"
    "      --max-group <N>              Samples per device pass [default: 64]\n"
    "  -t, --threads <THREADS>          Host BAM / VCF decode workers [default: min(16, hardware threads)]\n"
    "      --sequential                 Run CYP2D6 after the variant genes and the HLA genes of a group (the calls are the same)\n"
    "      --debug-reads                Also write read_debug.json into every sample's debug folder (needs an output_debug column that names one)\n"
    "  -v, --verbose...                 Enable verbose output (print the warnings and the timings of the batch)\n"
    "  -h, --help                       Print help\n"
    "\n"
    "Every sample's files are what `starphase_hip diplotype` takes for one sample; the debug folder is a manifest column (--output-debug is refused).\n"
    "Exit status: 0 when every sample was written, 65 when a sample failed (the others are written; each failure is printed with its row).\n";

int batch_clap_error(const std::string& m) {
    std::fprintf(stderr, "error: %s\n\nUsage: starphase_hip diplotype-batch [OPTIONS] --database <JSON> --reference <FASTA> --manifest <TSV>\n\nFor more information, try '--help'.\n", m.c_str());
    return EX_CLAP;
}

// one manifest row: the files of one sample
struct Row { int line = 0; std::string output, vcf, sample, sv_vcf, pharmcat, debug; std::vector<std::string> bams; };

std::vector<std::string> split(const std::string& s, char sep) {
    std::vector<std::string> out; size_t a = 0;
    for (;;) { const size_t b = s.find(sep, a); out.push_back(s.substr(a, b == std::string::npos ? std::string::npos : b - a)); if (b == std::string::npos) break; a = b + 1; }
    return out;
}

// create_dir_all; false with errno set when a component cannot be made
bool make_dirs(const std::string& dir) {
    std::string acc;
    for (size_t p = 0; p <= dir.size(); ++p) {
        if (p == dir.size() || dir[p] == '/') { if (!acc.empty() && !exists(acc) && ::mkdir(acc.c_str(), 0755) != 0) return false; }
        if (p < dir.size()) acc += dir[p];
    }
    return true;
}

int batch_main(int argc, char** argv) {
    sp_diplotype_settings s;
    sp_diplotype_settings_default(&s);
    std::string database, reference, manifest, include, exclude;
    uint64_t max_group = 0, threads = 0;
    int verbose = 0; bool debug_reads = false;
    for (int i = 2; i < argc; ++i) {
        std::string a = argv[i], val;
        bool has_inline = false;
        const size_t eq = a.find('=');
        if (a.rfind("--", 0) == 0 && eq != std::string::npos) { val = a.substr(eq + 1); a = a.substr(0, eq); has_inline = true; }
        auto need = [&](std::string* out) -> int {
            if (has_inline) { *out = val; return 0; }
            if (i + 1 >= argc) return batch_clap_error("a value is required for '" + a + "' but none was supplied");
            *out = argv[++i];
            return 0;
        };
        int rc = 0;
        std::string tmp;
        if (a == "-h" || a == "--help") { std::fputs(BATCH_HELP, stdout); return EX_OK_; }
        else if (a == "-d" || a == "--database") rc = need(&database);
        else if (a == "-r" || a == "--reference") rc = need(&reference);
        else if (a == "-m" || a == "--manifest") rc = need(&manifest);
        else if (a == "--include-set") rc = need(&include);
        else if (a == "--exclude-set") rc = need(&exclude);
        else if (a == "--disable-cdna-scoring") s.disable_cdna_scoring = 1;
        else if (a == "--hla-require-dna") s.hla_require_dna = 1;
        else if (a == "--debug-skip-hla") s.debug_skip_hla = 1;
        else if (a == "--infer-connections") s.infer_connections = 1;
        else if (a == "--normalize-d6-only") s.normalize_d6_only = 1;
        else if (a == "--sequential") s.sequential = 1;
        else if (a == "--debug-reads") debug_reads = true;
        else if (a == "-v" || a == "--verbose") ++verbose;
        else if (a.size() > 2 && a[0] == '-' && a[1] == 'v' && a.find_first_not_of('v', 1) == std::string::npos) verbose += (int)a.size() - 1;
        else if (a == "--max-sv-length" || a == "--min-consensus-count" || a == "--dual-max-ed-delta" || a == "-t" || a == "--threads" || a == "--max-group") {
            uint64_t v = 0;
            if ((rc = need(&tmp))) return rc;
            if (!parse_u64(tmp, &v)) return batch_clap_error("invalid value '" + tmp + "' for '" + a + "': invalid digit found in string");
            if (a == "--max-sv-length") s.max_sv_length = v;
            else if (a == "--min-consensus-count") s.min_consensus_count = v;
            else if (a == "--dual-max-ed-delta") s.dual_max_ed_delta = v;
            else if (a == "--max-group") max_group = v;
            else threads = v;
        } else if (a == "--max-error-rate" || a == "--min-cdf-prob" || a == "--expected-maf" || a == "--min-consensus-fraction") {
            double v = 0;
            if ((rc = need(&tmp))) return rc;
            if (!parse_f64(tmp, &v)) return batch_clap_error("invalid value '" + tmp + "' for '" + a + "': invalid float literal");
            if (a == "--max-error-rate") s.max_error_rate = v;
            else if (a == "--min-cdf-prob") s.min_cdf_prob = v;
            else if (a == "--expected-maf") s.expected_maf = v;
            else s.min_consensus_fraction = v;
        } else if (a == "--output-debug" || a == "-o" || a == "--output-calls" || a == "-c" || a == "--vcf" || a == "-b" || a == "--bam" || a == "-s" ||
                   a == "--sv-vcf" || a == "--sample-name" || a == "--pharmcat-tsv") {
            std::fprintf(stderr, "error: %s is a column of the manifest in diplotype-batch (one value per sample)\n", a.c_str());
            return EX_USAGE_;
        } else if (a == "--hla-revert-method" || a == "--output-cyp2d6-bam" || a == "--debug-hla-target") {
            std::fprintf(stderr, "error: %s is not supported by starphase_hip (the batch HLA method and the debug folder outputs listed in --help are)\n", a.c_str());
            return EX_USAGE_;
        } else return batch_clap_error("unexpected argument '" + a + "' found");
        if (rc) return rc;
        if (max_group > 0xFFFFFFFFull || threads > 0xFFFFFFFFull) return batch_clap_error("value too large for '" + a + "'");
    }
    std::string missing;
    if (database.empty()) missing += "\n  --database <JSON>";
    if (reference.empty()) missing += "\n  --reference <FASTA>";
    if (manifest.empty()) missing += "\n  --manifest <TSV>";
    if (!missing.empty()) return batch_clap_error("the following required arguments were not provided:" + missing);
    auto noinput = [](const std::string& where, const char* label, const std::string& p) {
        std::fprintf(stderr, "error: %s%s does not exist: \"%s\"\n", where.c_str(), label, p.c_str()); return EX_NOINPUT_; };
    if (!exists(database)) return noinput("", "Database JSON", database);
    if (!exists(reference)) return noinput("", "Reference FASTA", reference);
    if (!exists(manifest)) return noinput("", "Manifest", manifest);
    // the manifest
    std::vector<Row> rows;
    {
        FILE* f = std::fopen(manifest.c_str(), "rb");
        if (!f) { std::fprintf(stderr, "error: Error while reading manifest: %s\n", std::strerror(errno)); return EX_IOERR_; }
        std::string text; char buf[65536]; size_t got;
        while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
        std::fclose(f);
        int line_no = 0;
        for (std::string line : split(text, '\n')) {
            ++line_no;
            if (!line.empty() && line.back() == '\r') line.pop_back();
            if (line.empty() || line[0] == '#') continue;
            const std::vector<std::string> c = split(line, '\t');
            const int row_no = (int)rows.size() + 1;
            if (c.size() != 7) {
                std::fprintf(stderr, "error: manifest row %d (line %d): expected 7 tab-separated columns (output_calls, bams, vcf, sample_name, sv_vcf, pharmcat_tsv, output_debug), found %zu\n",
                             row_no, line_no, c.size());
                return EX_USAGE_;
            }
            auto field = [](const std::string& v) { return v == "-" ? std::string() : v; };
            Row r; r.line = line_no;
            r.output = field(c[0]); r.vcf = field(c[2]); r.sample = field(c[3]); r.sv_vcf = field(c[4]); r.pharmcat = field(c[5]); r.debug = field(c[6]);
            if (!field(c[1]).empty()) for (const std::string& b : split(c[1], ',')) if (!b.empty()) r.bams.push_back(b);
            if (r.output.empty()) { std::fprintf(stderr, "error: manifest row %d (line %d): output_calls is required\n", row_no, line_no); return EX_USAGE_; }
            rows.push_back(std::move(r));
        }
    }
    if (rows.empty()) { std::fprintf(stderr, "error: manifest \"%s\" lists no samples\n", manifest.c_str()); return EX_USAGE_; }
    if (debug_reads) {
        bool any = false;
        for (const Row& r : rows) any |= !r.debug.empty();
        if (!any) { std::fprintf(stderr, "error: --debug-reads needs a debug folder: no manifest row names one (output_debug)\n"); return EX_USAGE_; }
    }
    // every row through the checks of `diplotype`: the files (NOINPUT), then check_diplotype_settings (USAGE)
    std::vector<std::vector<const char*>> bam_ptrs(rows.size());
    std::vector<sp_sample_inputs> in(rows.size());
    for (size_t k = 0; k < rows.size(); ++k) {
        const Row& r = rows[k];
        const std::string where = "manifest row " + std::to_string(k + 1) + ": ";
        if (!r.vcf.empty() && !exists(r.vcf)) return noinput(where, "VCF file", r.vcf);
        if (!r.sv_vcf.empty() && !exists(r.sv_vcf)) return noinput(where, "SV VCF file", r.sv_vcf);
        for (const auto& b : r.bams) if (!exists(b)) return noinput(where, "Alignment file", b);
        for (const auto& b : r.bams) bam_ptrs[k].push_back(b.c_str());
        in[k] = sp_sample_inputs{};
        in[k].n_bams = (uint32_t)r.bams.size(); in[k].bams = bam_ptrs[k].data(); in[k].vcf = r.vcf.empty() ? nullptr : r.vcf.c_str();
        in[k].sv_vcf = r.sv_vcf.empty() ? nullptr : r.sv_vcf.c_str(); in[k].sample_name = r.sample.empty() ? nullptr : r.sample.c_str();
        sp_diplotype_settings sk = s;
        sk.include_set = include.empty() ? nullptr : include.c_str(); sk.exclude_set = exclude.empty() ? nullptr : exclude.c_str();
        char err[512];
        if (sp_diplotype_settings_check(&sk, &in[k], err, sizeof err) != SP_OK) {
            std::fprintf(stderr, "error: %sError while processing CLI settings: %s\n", where.c_str(), err);
            return EX_USAGE_;
        }
    }
    if (s.disable_cdna_scoring) s.hla_require_dna = 1;       // what the check sets for a sample with BAMs (the HLA genes only run for those)
    if (!include.empty() && !exists(include)) return noinput("", "Include set", include);
    if (!exclude.empty() && !exists(exclude)) return noinput("", "Exclude set", exclude);
    std::vector<const char*> debug(rows.size(), nullptr);
    bool any_debug = false;
    for (size_t k = 0; k < rows.size(); ++k) {
        if (rows[k].debug.empty()) continue;
        if (!make_dirs(rows[k].debug)) { std::fprintf(stderr, "error: manifest row %zu: Error while creating debug folder: %s\n", k + 1, std::strerror(errno)); return EX_IOERR_; }
        debug[k] = rows[k].debug.c_str(); any_debug = true;
    }
    s.include_set = include.empty() ? nullptr : include.c_str(); s.exclude_set = exclude.empty() ? nullptr : exclude.c_str();
    // the device work
    sp_starphase* h = nullptr;
    int32_t rc = sp_starphase_create(nullptr, database.c_str(), reference.c_str(), &s, &h);
    if (rc != SP_OK) {
        std::fprintf(stderr, "error: %s\n", sp_starphase_last_error(nullptr));
        return rc == SP_ERR_NO_DEVICE || rc == SP_ERR_HIP ? EX_UNAVAILABLE_ : EX_IOERR_;
    }
    if (debug_reads) sp_starphase_set_read_debug(h, 1);
    sp_batch_options o{};
    o.max_group = (uint32_t)max_group; o.decode_threads = (uint32_t)threads;
    std::vector<sp_result*> out(rows.size(), nullptr);
    std::vector<int32_t> rcs(rows.size(), SP_OK);
    sp_starphase_call_batch(h, (uint32_t)rows.size(), in.data(), any_debug ? debug.data() : nullptr, &o, out.data(), rcs.data());
    int code = EX_OK_; bool failed = false;
    for (size_t k = 0; k < rows.size(); ++k) {
        const char* warn = sp_starphase_sample_warnings(h, (uint32_t)k);
        if (warn && *warn && (verbose || rcs[k] != SP_OK)) std::fprintf(stderr, "manifest row %zu: %s", k + 1, warn);
        if (rcs[k] != SP_OK || !out[k]) {
            std::fprintf(stderr, "error: manifest row %zu: Error while calling diplotypes: %s\n", k + 1, sp_starphase_sample_error(h, (uint32_t)k));
            failed = true;
            continue;
        }
        if (sp_result_save(out[k], rows[k].output.c_str()) != SP_OK) {
            std::fprintf(stderr, "error: manifest row %zu: Error while writing diplotypes to file: %s\n", k + 1, sp_result_last_error(out[k]));
            code = EX_IOERR_;
        } else if (!rows[k].pharmcat.empty() && sp_result_save_pharmcat_tsv(out[k], rows[k].pharmcat.c_str()) != SP_OK) {
            std::fprintf(stderr, "error: manifest row %zu: Error while writing PharmCAT diplotypes to file: %s\n", k + 1, sp_result_last_error(out[k]));
            code = EX_IOERR_;
        }
        sp_result_free(out[k]);
    }
    if (verbose) {
        sp_starphase_batch_timing t{};
        sp_starphase_last_batch_timing(h, &t);
        std::fprintf(stderr, "batch %.1f ms for %u samples in %u groups, %u failed (decode %.1f, variant genes %.1f, HLA %.1f with %llu reads, CYP2D6 %.1f with %llu reads, "
                     "packaging %.1f)\n", t.wall_ms, t.n_samples, t.n_groups, t.n_failed, t.decode_ms, t.variant_ms, t.hla_ms, (unsigned long long)t.n_hla_reads, t.cyp_ms,
                     (unsigned long long)t.n_cyp_reads, t.package_ms);
    }
    sp_starphase_free(h);
    return code != EX_OK_ ? code : failed ? EX_DATAERR_ : EX_OK_;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2 || !std::strcmp(argv[1], "-h") || !std::strcmp(argv[1], "--help")) {
        std::printf("starphase_hip: PGx diplotyping on AMD Instinct GPUs\n\nUsage: starphase_hip <COMMAND> [OPTIONS]\n\nCommands:\n  diplotype        Diplotype a sample from its files\n"
                    "  diplotype-batch  Diplotype the samples of a manifest, many per device pass\n");
        return argc < 2 ? EX_CLAP : EX_OK_;
    }
    if (!std::strcmp(argv[1], "diplotype-batch")) return batch_main(argc, argv);
    if (std::strcmp(argv[1], "diplotype") != 0) return clap_error(std::string("unrecognized subcommand '") + argv[1] + "'");
    sp_diplotype_settings s;
    sp_diplotype_settings_default(&s);
    std::string database, reference, vcf, sv_vcf, output, pharmcat, include, exclude, debug, sample;
    std::vector<std::string> bams;
    int verbose = 0; bool debug_reads = false;
    for (int i = 2; i < argc; ++i) {
        std::string a = argv[i], val;
        bool has_inline = false;
        const size_t eq = a.find('=');
        if (a.rfind("--", 0) == 0 && eq != std::string::npos) { val = a.substr(eq + 1); a = a.substr(0, eq); has_inline = true; }
        auto value = [&](std::string* out) -> bool {
            if (has_inline) { *out = val; return true; }
            if (i + 1 >= argc) return false;
            *out = argv[++i];
            return true;
        };
        auto need = [&](std::string* out) -> int {
            return value(out) ? 0 : clap_error("a value is required for '" + a + "' but none was supplied");
        };
        int rc = 0;
        std::string tmp;
        if (a == "-h" || a == "--help") { std::fputs(HELP, stdout); return EX_OK_; }
        else if (a == "-d" || a == "--database") rc = need(&database);
        else if (a == "-r" || a == "--reference") rc = need(&reference);
        else if (a == "-c" || a == "--vcf") rc = need(&vcf);
        else if (a == "-s" || a == "--sv-vcf") rc = need(&sv_vcf);
        else if (a == "-b" || a == "--bam") { rc = need(&tmp); if (!rc) bams.push_back(tmp); }
        else if (a == "-o" || a == "--output-calls") rc = need(&output);
        else if (a == "--pharmcat-tsv") rc = need(&pharmcat);
        else if (a == "--include-set") rc = need(&include);
        else if (a == "--exclude-set") rc = need(&exclude);
        else if (a == "--output-debug") rc = need(&debug);
        else if (a == "--sample-name") rc = need(&sample);
        else if (a == "--disable-cdna-scoring") s.disable_cdna_scoring = 1;
        else if (a == "--hla-require-dna") s.hla_require_dna = 1;
        else if (a == "--debug-skip-hla") s.debug_skip_hla = 1;
        else if (a == "--infer-connections") s.infer_connections = 1;
        else if (a == "--normalize-d6-only") s.normalize_d6_only = 1;
        else if (a == "--sequential") s.sequential = 1;
        else if (a == "--debug-reads") debug_reads = true;
        else if (a == "-v" || a == "--verbose") ++verbose;
        else if (a.size() > 2 && a[0] == '-' && a[1] == 'v' && a.find_first_not_of('v', 1) == std::string::npos) verbose += (int)a.size() - 1;
        else if (a == "--max-sv-length" || a == "--min-consensus-count" || a == "--dual-max-ed-delta" || a == "-t" || a == "--threads") {
            uint64_t v = 0;
            if ((rc = need(&tmp))) return rc;
            if (!parse_u64(tmp, &v)) return clap_error("invalid value '" + tmp + "' for '" + a + "': invalid digit found in string");
            if (a == "--max-sv-length") s.max_sv_length = v;
            else if (a == "--min-consensus-count") s.min_consensus_count = v;
            else if (a == "--dual-max-ed-delta") s.dual_max_ed_delta = v;
        } else if (a == "--max-error-rate" || a == "--min-cdf-prob" || a == "--expected-maf" || a == "--min-consensus-fraction") {
            double v = 0;
            if ((rc = need(&tmp))) return rc;
            if (!parse_f64(tmp, &v)) return clap_error("invalid value '" + tmp + "' for '" + a + "': invalid float literal");
            if (a == "--max-error-rate") s.max_error_rate = v;
            else if (a == "--min-cdf-prob") s.min_cdf_prob = v;
            else if (a == "--expected-maf") s.expected_maf = v;
            else s.min_consensus_fraction = v;
        } else if (a == "--hla-revert-method" || a == "--output-cyp2d6-bam" || a == "--debug-hla-target") {
            std::fprintf(stderr, "error: %s is not supported by starphase_hip (the batch HLA method and the debug folder outputs listed in --help are)\n", a.c_str());
            return EX_USAGE_;
        } else return clap_error("unexpected argument '" + a + "' found");
        if (rc) return rc;
    }
    std::string missing;
    if (database.empty()) missing += "\n  --database <JSON>";
    if (reference.empty()) missing += "\n  --reference <FASTA>";
    if (output.empty()) missing += "\n  --output-calls <JSON>";
    if (!missing.empty()) return clap_error("the following required arguments were not provided:" + missing);
    // check_diplotype_settings (src/cli/diplotype.rs:200-330): the files first (check_required_filename exits with NOINPUT), then the rules
    auto noinput = [](const char* label, const std::string& p) { std::fprintf(stderr, "error: %s does not exist: \"%s\"\n", label, p.c_str()); return EX_NOINPUT_; };
    if (!exists(database)) return noinput("Database JSON", database);
    if (!exists(reference)) return noinput("Reference FASTA", reference);
    if (!vcf.empty() && !exists(vcf)) return noinput("VCF file", vcf);
    if (!sv_vcf.empty() && !exists(sv_vcf)) return noinput("SV VCF file", sv_vcf);
    for (const auto& b : bams) if (!exists(b)) return noinput("Alignment file", b);
    std::vector<const char*> bam_ptrs;
    for (const auto& b : bams) bam_ptrs.push_back(b.c_str());
    sp_sample_inputs in{};
    in.n_bams = (uint32_t)bams.size(); in.bams = bam_ptrs.data(); in.vcf = vcf.empty() ? nullptr : vcf.c_str();
    s.include_set = include.empty() ? nullptr : include.c_str(); s.exclude_set = exclude.empty() ? nullptr : exclude.c_str();
    s.sample_name = sample.empty() ? nullptr : sample.c_str(); s.sv_vcf = sv_vcf.empty() ? nullptr : sv_vcf.c_str();
    s.debug_folder = debug.empty() ? nullptr : debug.c_str();
    if (debug_reads && debug.empty()) { std::fprintf(stderr, "error: --debug-reads needs a debug folder (--output-debug <DIR>)\n"); return EX_USAGE_; }
    char err[512];
    if (sp_diplotype_settings_check(&s, &in, err, sizeof err) != SP_OK) {
        std::fprintf(stderr, "error: Error while processing CLI settings: %s\n", err);
        return EX_USAGE_;
    }
    if (!include.empty() && !exists(include)) return noinput("Include set", include);
    if (!exclude.empty() && !exists(exclude)) return noinput("Exclude set", exclude);
    if (!debug.empty()) {
        std::string acc;                                   // create_dir_all
        for (size_t p = 0; p <= debug.size(); ++p) {
            if (p == debug.size() || debug[p] == '/') { if (!acc.empty() && !exists(acc) && ::mkdir(acc.c_str(), 0755) != 0) {
                std::fprintf(stderr, "error: Error while creating debug folder: %s\n", std::strerror(errno)); return EX_IOERR_; } }
            if (p < debug.size()) acc += debug[p];
        }
    }
    // the device work
    sp_starphase* h = nullptr;
    int32_t rc = sp_starphase_create(nullptr, database.c_str(), reference.c_str(), &s, &h);
    if (rc != SP_OK) {
        std::fprintf(stderr, "error: %s\n", sp_starphase_last_error(nullptr));
        return rc == SP_ERR_NO_DEVICE || rc == SP_ERR_HIP ? EX_UNAVAILABLE_ : EX_IOERR_;
    }
    if (debug_reads) sp_starphase_set_read_debug(h, 1);
    sp_result* result = nullptr;
    rc = sp_starphase_call(h, &in, &result);
    const char* warn = sp_starphase_warnings(h);
    if (warn && *warn) std::fprintf(stderr, "%s", warn);
    if (rc != SP_OK) {
        std::fprintf(stderr, "error: Error while calling diplotypes: %s\n", sp_starphase_last_error(h));
        sp_starphase_free(h);
        return EX_DATAERR_;
    }
    if (verbose) {
        sp_starphase_timing t{};
        sp_starphase_last_timing(h, &t);
        std::fprintf(stderr, "call %.1f ms (BAM decode %.1f, variant genes %.1f, HLA %.1f with %u reads, CYP2D6 %.1f with %u reads)\n", t.call_ms, t.bam_decode_ms,
                     t.variant_ms, t.hla_ms, t.n_hla_reads, t.cyp_ms, t.n_cyp_reads);
    }
    int code = EX_OK_;
    if (sp_result_save(result, output.c_str()) != SP_OK) {
        std::fprintf(stderr, "error: Error while writing diplotypes to file: %s\n", sp_result_last_error(result));
        code = EX_IOERR_;
    } else if (!pharmcat.empty() && sp_result_save_pharmcat_tsv(result, pharmcat.c_str()) != SP_OK) {
        std::fprintf(stderr, "error: Error while writing PharmCAT diplotypes to file: %s\n", sp_result_last_error(result));
        code = EX_IOERR_;
    }
    sp_result_free(result);
    sp_starphase_free(h);
    return code;
}

// starphase_hip_cli.cpp -- `starphase_hip diplotype ...`: the reference's `pbstarphase diplotype` command (src/main.rs, src/cli/diplotype.rs) on
// libstarphase_hip.  Flag names and defaults are the reference's for everything sp_starphase_call supports; exit codes as the reference's:
// 2 for a command line that does not parse (clap), NOINPUT (66) for an input file that does not exist, USAGE (64) when check_diplotype_settings
// refuses the settings, IOERR (74) for the database / reference / output files, DATAERR (65) when the call fails.  Every check of the command
// line is made before the first device call.
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

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2 || !std::strcmp(argv[1], "-h") || !std::strcmp(argv[1], "--help")) {
        std::printf("starphase_hip: PGx diplotyping on AMD Instinct GPUs\n\nUsage: starphase_hip diplotype [OPTIONS]\n\nCommands:\n  diplotype  Diplotype a sample from its files\n");
        return argc < 2 ? EX_CLAP : EX_OK_;
    }
    if (std::strcmp(argv[1], "diplotype") != 0) return clap_error(std::string("unrecognized subcommand '") + argv[1] + "'");
    sp_diplotype_settings s;
    sp_diplotype_settings_default(&s);
    std::string database, reference, vcf, sv_vcf, output, pharmcat, include, exclude, debug, sample;
    std::vector<std::string> bams;
    int verbose = 0;
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

// starphase_hip_cli.cpp -- `starphase_hip diplotype ...`: the reference's `pbstarphase diplotype` command (src/main.rs, src/cli/diplotype.rs) on
// libstarphase_hip.  Flag names and defaults are the reference's for everything sp_starphase_call supports; exit codes as the reference's:
// 2 for a command line that does not parse (clap), NOINPUT (66) for an input file that does not exist, USAGE (64) when check_diplotype_settings
// refuses the settings, IOERR (74) for the database / reference / output files, DATAERR (65) when the call fails.  Every check of the command
// line is made before the first device call.  `starphase_hip diplotype-batch` types the samples of a manifest through sp_starphase_call_batch.
// `starphase_hip update-hla` rebuilds a database's HLA section from the two FASTA files of an IMGT/HLA release (the HLA half of `pbstarphase build`, offline).
#include "../../include/starphase_hip.h"
#include <sys/stat.h>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

namespace {

enum { EX_OK_ = 0, EX_CLAP = 2, EX_USAGE_ = 64, EX_DATAERR_ = 65, EX_NOINPUT_ = 66, EX_UNAVAILABLE_ = 69, EX_IOERR_ = 74 };

const char* USAGE = "starphase_hip diplotype [OPTIONS] --database <JSON> --reference <FASTA> --output-calls <JSON>";
const char* BATCH_USAGE = "starphase_hip diplotype-batch [OPTIONS] --database <JSON> --reference <FASTA> --manifest <TSV>";

// the help texts: each command's own head and Execution section around the sections of the options both take
const char* HELP_HEAD =
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
    "      --debug-hla-mappings         Fill hla_debug.json's mapping_stats: each HLA consensus against every allowed allele, CIGAR and MD (needs --output-debug)\n"
    "      --debug-hla-ties             Also write hla_ties.json: for each HLA consensus the alleles its call cannot tell from the winner -- equal, score_only, beats_winner (needs --output-debug)\n"
    "      --debug-consensus-support    Also write consensus_support.json: how the member reads back each HLA consensus, column by column (needs --output-debug)\n"
    "      --debug-cyp2d6-support       Also write cyp2d6_consensus_support.json: the same for each CYP2D6 consensus region (needs --output-debug)\n"
    "      --debug-cyp2d6-vcf           Also write cyp2d6_alleles.vcf.gz: the variants of the CYP2D6 regions, with the member reads that span (SR) and agree with (CR) each (needs --output-debug)\n"
    "      --debug-cyp2d6-alternatives  Also write cyp2d6_alternatives.json: the ten best CYP2D6 chain pairs with their scores, score components and coverage (needs --output-debug)\n"
    "      --debug-cyp2d6-alternative-reads  Also write cyp2d6_alternative_reads.json: those pairs read by read (which reads decide between them, which are unmet) and the observed-chain table (needs --output-debug)\n"
    "      --debug-variant-alternatives Also write variant_alternatives.json: the ten best diplotypes of every variant gene with their scores and their missing and unexpected variants (needs --output-debug)\n"
    "      --debug-support-insertions   Those two files also list the inserted strings behind the columns their insertions contest (with one of the two switches above)\n"
    "      --debug-support-haplotypes   Those two files also list the read haplotypes: the patterns of calls the reads make at the contested columns (with one of the two switches above)\n"
    "      --sample-name <STRING>       Sample name from the input VCFs (default: first sample)\n"
    "\n";
const char* BATCH_HELP_HEAD =
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
    "\n";
const char* HELP_SHARED =
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
    "\n";
const char* HELP_TAIL =
    "Execution:\n"
    "      --sequential                 Run the variant genes, the HLA genes and CYP2D6 one after another (the calls are the same)\n"
    "  -t, --threads <THREADS>          Accepted for compatibility; the reference deprecates it [default: 1]\n"
    "  -v, --verbose...                 Enable verbose output (print the warnings and timings of the call)\n"
    "  -h, --help                       Print help\n"
    "\n"
    "Not supported here: --hla-revert-method, --output-cyp2d6-bam, --debug-hla-target\n";
const char* BATCH_HELP_TAIL =
    "Execution:\n"
    "      --max-group <N>              Samples per device pass [default: 64]\n"
    "  -t, --threads <THREADS>          Host BAM / VCF decode workers [default: min(16, hardware threads)]\n"
    "      --sequential                 Run CYP2D6 after the variant genes and the HLA genes of a group (the calls are the same)\n"
    "      --debug-reads                Also write read_debug.json into every sample's debug folder (needs an output_debug column that names one)\n"
    "      --debug-hla-mappings         Fill the mapping_stats of every sample's hla_debug.json (needs an output_debug column that names a folder)\n"
    "      --debug-hla-ties             Also write every sample's hla_ties.json: the alleles each HLA call cannot tell from its winner (needs an output_debug column that names a folder)\n"
    "      --debug-consensus-support    Also write every sample's consensus_support.json (needs an output_debug column that names a folder)\n"
    "      --debug-cyp2d6-support       Also write every sample's cyp2d6_consensus_support.json (needs an output_debug column that names a folder)\n"
    "      --debug-cyp2d6-vcf           Also write every sample's cyp2d6_alleles.vcf.gz (needs an output_debug column that names a folder)\n"
    "      --debug-cyp2d6-alternatives  Also write every sample's cyp2d6_alternatives.json (needs an output_debug column that names a folder)\n"
    "      --debug-cyp2d6-alternative-reads  Also write every sample's cyp2d6_alternative_reads.json (needs an output_debug column that names a folder)\n"
    "      --debug-variant-alternatives Also write every sample's variant_alternatives.json (needs an output_debug column that names a folder)\n"
    "      --debug-support-insertions   Those two files also list the inserted strings behind the columns their insertions contest (with one of the two switches above)\n"
    "      --debug-support-haplotypes   Those two files also list the read haplotypes: the patterns of calls the reads make at the contested columns (with one of the two switches above)\n"
    "  -v, --verbose...                 Enable verbose output (print the warnings and the timings of the batch)\n"
    "  -h, --help                       Print help\n"
    "\n"
    "Every sample's files are what `starphase_hip diplotype` takes for one sample; the debug folder is a manifest column (--output-debug is refused).\n"
    "Exit status: 0 when every sample was written, 65 when a sample failed (the others are written; each failure is printed with its row).\n";

const char* UPDATE_USAGE = "starphase_hip update-hla [OPTIONS] --database <JSON> --reference <FASTA> --hla-gen <FASTA> --hla-nuc <FASTA> --output-db <JSON>";
const char* UPDATE_HELP =
    "Rebuild a database's HLA section from the FASTA files of an IMGT/HLA release (the HLA half of pbstarphase build, offline)\n"
    "\n"
    "Usage: starphase_hip update-hla [OPTIONS] --database <JSON> --reference <FASTA> --hla-gen <FASTA> --hla-nuc <FASTA> --output-db <JSON>\n"
    "\n"
    "Input/Output:\n"
    "  -d, --database <JSON>            Input database file (JSON); its hla_config gives the starting gene coordinates (HLA-A / HLA-B defaults without one)\n"
    "  -r, --reference <FASTA>          Reference FASTA file\n"
    "      --hla-gen <FASTA>            Genomic allele sequences of the release (hla_gen.fasta, plain or gzip)\n"
    "      --hla-nuc <FASTA>            cDNA allele sequences of the release (hla_nuc.fasta, plain or gzip)\n"
    "      --hla-version <STRING>       Version string stored as database_metadata.hla_version [default: the input database's]\n"
    "  -o, --output-db <JSON>           Output database file (JSON; gzip when the name ends in .gz)\n"
    "\n"
    "Execution:\n"
    "      --batch-alleles <N>          Alleles per device pass [default: 1024]\n"
    "  -v, --verbose...                 Enable verbose output (print the warnings, every gene's coordinates and its worst mapping)\n"
    "  -h, --help                       Print help\n"
    "\n"
    "CPIC and PharmVar sections are carried over unchanged (the reference builds them from the network).\n";

bool exists(const std::string& p) { struct stat st; return ::stat(p.c_str(), &st) == 0; }

int clap_error(const char* usage, const std::string& m) {
    std::fprintf(stderr, "error: %s\n\nUsage: %s\n\nFor more information, try '--help'.\n", m.c_str(), usage);
    return EX_CLAP;
}

int noinput(const std::string& where, const char* label, const std::string& p) {
    std::fprintf(stderr, "error: %s%s does not exist: \"%s\"\n", where.c_str(), label, p.c_str());
    return EX_NOINPUT_;
}

bool parse_f64(const std::string& s, double* out) { char* end = nullptr; errno = 0; *out = std::strtod(s.c_str(), &end); return !s.empty() && end && *end == 0 && errno == 0; }
bool parse_u64(const std::string& s, uint64_t* out) {
    if (s.empty() || s[0] == '-' || s[0] == '+') return false;
    char* end = nullptr; errno = 0; *out = std::strtoull(s.c_str(), &end, 10); return end && *end == 0 && errno == 0;
}

// the options both commands take
struct Options {
    sp_diplotype_settings s;
    std::string database, reference, include, exclude;
    int verbose = 0; bool debug_reads = false, debug_hla_mappings = false, debug_hla_ties = false, debug_consensus_support = false, debug_cyp2d6_support = false, debug_cyp2d6_vcf = false, debug_cyp2d6_alternatives = false, debug_cyp2d6_alternative_reads = false, debug_variant_alternatives = false, debug_support_insertions = false, debug_support_haplotypes = false;
};

// the option being parsed: its name (a `--key=value` split) and where its value comes from.  need*: 0, or the exit status of the clap error
struct Arg {
    int argc; char** argv; int i; const char* usage;
    std::string a, val; bool has_inline = false;
    int need(std::string* out) {
        if (has_inline) { *out = val; return 0; }
        if (i + 1 >= argc) return clap_error(usage, "a value is required for '" + a + "' but none was supplied");
        *out = argv[++i];
        return 0;
    }
    int need_u64(uint64_t* v) {
        std::string tmp;
        if (int rc = need(&tmp)) return rc;
        return parse_u64(tmp, v) ? 0 : clap_error(usage, "invalid value '" + tmp + "' for '" + a + "': invalid digit found in string");
    }
    int need_f64(double* v) {
        std::string tmp;
        if (int rc = need(&tmp)) return rc;
        return parse_f64(tmp, v) ? 0 : clap_error(usage, "invalid value '" + tmp + "' for '" + a + "': invalid float literal");
    }
};

// argv[2..] of either command.  own(arg): the options only that command has -- NOT_MINE, 0 when it took the option, else the exit status.
// Returns PARSED, or the exit status (0 after --help).
enum { PARSED = -1, NOT_MINE = -2 };
int parse_options(int argc, char** argv, const char* usage, const std::string& help, Options& o, const std::function<int(Arg&)>& own) {
    sp_diplotype_settings& s = o.s;
    Arg arg{argc, argv, 2, usage};
    for (int& i = arg.i; i < argc; ++i) {
        std::string& a = arg.a;
        a = argv[i]; arg.has_inline = false;
        const size_t eq = a.find('=');
        if (a.rfind("--", 0) == 0 && eq != std::string::npos) { arg.val = a.substr(eq + 1); a = a.substr(0, eq); arg.has_inline = true; }
        int rc = 0;
        uint64_t u = 0; double f = 0;
        if (a == "-h" || a == "--help") { std::fputs(help.c_str(), stdout); return EX_OK_; }
        else if (a == "-d" || a == "--database") rc = arg.need(&o.database);
        else if (a == "-r" || a == "--reference") rc = arg.need(&o.reference);
        else if (a == "--include-set") rc = arg.need(&o.include);
        else if (a == "--exclude-set") rc = arg.need(&o.exclude);
        else if (a == "--disable-cdna-scoring") s.disable_cdna_scoring = 1;
        else if (a == "--hla-require-dna") s.hla_require_dna = 1;
        else if (a == "--debug-skip-hla") s.debug_skip_hla = 1;
        else if (a == "--infer-connections") s.infer_connections = 1;
        else if (a == "--normalize-d6-only") s.normalize_d6_only = 1;
        else if (a == "--sequential") s.sequential = 1;
        else if (a == "--debug-reads") o.debug_reads = true;
        else if (a == "--debug-hla-mappings") o.debug_hla_mappings = true;
        else if (a == "--debug-hla-ties") o.debug_hla_ties = true;
        else if (a == "--debug-consensus-support") o.debug_consensus_support = true;
        else if (a == "--debug-cyp2d6-support") o.debug_cyp2d6_support = true;
        else if (a == "--debug-cyp2d6-vcf") o.debug_cyp2d6_vcf = true;
        else if (a == "--debug-cyp2d6-alternatives") o.debug_cyp2d6_alternatives = true;
        else if (a == "--debug-cyp2d6-alternative-reads") o.debug_cyp2d6_alternative_reads = true;
        else if (a == "--debug-variant-alternatives") o.debug_variant_alternatives = true;
        else if (a == "--debug-support-insertions") o.debug_support_insertions = true;
        else if (a == "--debug-support-haplotypes") o.debug_support_haplotypes = true;
        else if (a == "-v" || a == "--verbose") ++o.verbose;
        else if (a.size() > 2 && a[0] == '-' && a[1] == 'v' && a.find_first_not_of('v', 1) == std::string::npos) o.verbose += (int)a.size() - 1;
        else if (a == "--max-sv-length") { if (!(rc = arg.need_u64(&u))) s.max_sv_length = u; }
        else if (a == "--min-consensus-count") { if (!(rc = arg.need_u64(&u))) s.min_consensus_count = u; }
        else if (a == "--dual-max-ed-delta") { if (!(rc = arg.need_u64(&u))) s.dual_max_ed_delta = u; }
        else if (a == "--max-error-rate") { if (!(rc = arg.need_f64(&f))) s.max_error_rate = f; }
        else if (a == "--min-cdf-prob") { if (!(rc = arg.need_f64(&f))) s.min_cdf_prob = f; }
        else if (a == "--expected-maf") { if (!(rc = arg.need_f64(&f))) s.expected_maf = f; }
        else if (a == "--min-consensus-fraction") { if (!(rc = arg.need_f64(&f))) s.min_consensus_fraction = f; }
        else if ((rc = own(arg)) != NOT_MINE) {}
        else if (a == "--hla-revert-method" || a == "--output-cyp2d6-bam" || a == "--debug-hla-target") {
            std::fprintf(stderr, "error: %s is not supported by starphase_hip (the batch HLA method and the debug folder outputs listed in --help are)\n", a.c_str());
            return EX_USAGE_;
        } else return clap_error(usage, "unexpected argument '" + a + "' found");
        if (rc) return rc;
    }
    return PARSED;
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

// the handle of the parsed options (o.s complete), or NULL and the exit status: UNAVAILABLE without a device, IOERR for what it loads
sp_starphase* create_handle(const Options& o, int* code) {
    sp_starphase* h = nullptr;
    const int32_t rc = sp_starphase_create(nullptr, o.database.c_str(), o.reference.c_str(), &o.s, &h);
    if (rc != SP_OK) {
        std::fprintf(stderr, "error: %s\n", sp_starphase_last_error(nullptr));
        *code = rc == SP_ERR_NO_DEVICE || rc == SP_ERR_HIP ? EX_UNAVAILABLE_ : EX_IOERR_;
        return nullptr;
    }
    if (o.debug_reads) sp_starphase_set_read_debug(h, 1);
    if (o.debug_hla_mappings) sp_starphase_set_hla_debug_mappings(h, 1);
    if (o.debug_hla_ties) sp_starphase_set_hla_ties(h, 1);
    if (o.debug_consensus_support) sp_starphase_set_consensus_support(h, 1);
    if (o.debug_cyp2d6_support) sp_starphase_set_cyp_consensus_support(h, 1);
    if (o.debug_cyp2d6_vcf) sp_starphase_set_cyp_vcf(h, 1);
    if (o.debug_cyp2d6_alternatives) sp_starphase_set_cyp_alternatives(h, 1);
    if (o.debug_cyp2d6_alternative_reads) sp_starphase_set_cyp_alternative_reads(h, 1);
    if (o.debug_variant_alternatives) sp_starphase_set_variant_alternatives(h, 1);
    if (o.debug_support_insertions) sp_starphase_set_support_insertions(h, 1);
    if (o.debug_support_haplotypes) sp_starphase_set_support_haplotypes(h, 1);
    return h;
}

// the calls JSON and, when named, the PharmCAT TSV of one result
int save_result(sp_result* result, const std::string& where, const std::string& output, const std::string& pharmcat) {
    if (sp_result_save(result, output.c_str()) != SP_OK) {
        std::fprintf(stderr, "error: %sError while writing diplotypes to file: %s\n", where.c_str(), sp_result_last_error(result));
        return EX_IOERR_;
    }
    if (!pharmcat.empty() && sp_result_save_pharmcat_tsv(result, pharmcat.c_str()) != SP_OK) {
        std::fprintf(stderr, "error: %sError while writing PharmCAT diplotypes to file: %s\n", where.c_str(), sp_result_last_error(result));
        return EX_IOERR_;
    }
    return EX_OK_;
}

// one manifest row: the files of one sample
struct Row { int line = 0; std::string output, vcf, sample, sv_vcf, pharmcat, debug; std::vector<std::string> bams; };

std::vector<std::string> split(const std::string& s, char sep) {
    std::vector<std::string> out; size_t a = 0;
    for (;;) { const size_t b = s.find(sep, a); out.push_back(s.substr(a, b == std::string::npos ? std::string::npos : b - a)); if (b == std::string::npos) break; a = b + 1; }
    return out;
}

int batch_main(int argc, char** argv) {
    Options o;
    sp_diplotype_settings& s = o.s;
    sp_diplotype_settings_default(&s);
    const std::string &database = o.database, &reference = o.reference, &include = o.include, &exclude = o.exclude;
    std::string manifest;
    uint64_t max_group = 0, threads = 0;
    const int parsed = parse_options(argc, argv, BATCH_USAGE, std::string(BATCH_HELP_HEAD) + HELP_SHARED + BATCH_HELP_TAIL, o, [&](Arg& arg) -> int {
        const std::string& a = arg.a;
        if (a == "-m" || a == "--manifest") return arg.need(&manifest);
        if (a == "-t" || a == "--threads" || a == "--max-group") {
            if (int rc = arg.need_u64(a == "--max-group" ? &max_group : &threads)) return rc;
            return max_group > 0xFFFFFFFFull || threads > 0xFFFFFFFFull ? clap_error(BATCH_USAGE, "value too large for '" + a + "'") : 0;
        }
        if (a == "--output-debug" || a == "-o" || a == "--output-calls" || a == "-c" || a == "--vcf" || a == "-b" || a == "--bam" || a == "-s" ||
            a == "--sv-vcf" || a == "--sample-name" || a == "--pharmcat-tsv") {
            std::fprintf(stderr, "error: %s is a column of the manifest in diplotype-batch (one value per sample)\n", a.c_str());
            return EX_USAGE_;
        }
        return NOT_MINE;
    });
    if (parsed != PARSED) return parsed;
    const int verbose = o.verbose; const bool debug_reads = o.debug_reads, debug_hla_mappings = o.debug_hla_mappings, debug_hla_ties = o.debug_hla_ties, debug_consensus_support = o.debug_consensus_support, debug_cyp2d6_support = o.debug_cyp2d6_support, debug_cyp2d6_vcf = o.debug_cyp2d6_vcf, debug_cyp2d6_alternatives = o.debug_cyp2d6_alternatives, debug_cyp2d6_alternative_reads = o.debug_cyp2d6_alternative_reads, debug_variant_alternatives = o.debug_variant_alternatives;
    std::string missing;
    if (database.empty()) missing += "\n  --database <JSON>";
    if (reference.empty()) missing += "\n  --reference <FASTA>";
    if (manifest.empty()) missing += "\n  --manifest <TSV>";
    if (!missing.empty()) return clap_error(BATCH_USAGE, "the following required arguments were not provided:" + missing);
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
    if (debug_reads || debug_hla_mappings || debug_hla_ties || debug_consensus_support || debug_cyp2d6_support || debug_cyp2d6_vcf || debug_cyp2d6_alternatives || debug_cyp2d6_alternative_reads || debug_variant_alternatives) {
        bool any = false;
        for (const Row& r : rows) any |= !r.debug.empty();
        if (!any) { std::fprintf(stderr, "error: %s needs a debug folder: no manifest row names one (output_debug)\n", debug_reads ? "--debug-reads" : debug_hla_mappings ? "--debug-hla-mappings" : debug_hla_ties ? "--debug-hla-ties" : debug_consensus_support ? "--debug-consensus-support" : debug_cyp2d6_support ? "--debug-cyp2d6-support" : debug_cyp2d6_vcf ? "--debug-cyp2d6-vcf" : debug_cyp2d6_alternatives ? "--debug-cyp2d6-alternatives" : debug_cyp2d6_alternative_reads ? "--debug-cyp2d6-alternative-reads" : "--debug-variant-alternatives"); return EX_USAGE_; }
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
    int code = EX_OK_;
    sp_starphase* h = create_handle(o, &code);
    if (!h) return code;
    sp_batch_options bo{};
    bo.max_group = (uint32_t)max_group; bo.decode_threads = (uint32_t)threads;
    std::vector<sp_result*> out(rows.size(), nullptr);
    std::vector<int32_t> rcs(rows.size(), SP_OK);
    sp_starphase_call_batch(h, (uint32_t)rows.size(), in.data(), any_debug ? debug.data() : nullptr, &bo, out.data(), rcs.data());
    bool failed = false;
    for (size_t k = 0; k < rows.size(); ++k) {
        const char* warn = sp_starphase_sample_warnings(h, (uint32_t)k);
        if (warn && *warn && (verbose || rcs[k] != SP_OK)) std::fprintf(stderr, "manifest row %zu: %s", k + 1, warn);
        if (rcs[k] != SP_OK || !out[k]) {
            std::fprintf(stderr, "error: manifest row %zu: Error while calling diplotypes: %s\n", k + 1, sp_starphase_sample_error(h, (uint32_t)k));
            failed = true;
            continue;
        }
        if (save_result(out[k], "manifest row " + std::to_string(k + 1) + ": ", rows[k].output, rows[k].pharmcat) != EX_OK_) code = EX_IOERR_;
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

int update_hla_main(int argc, char** argv) {
    std::string database, reference, gen, nuc, version, output;
    bool has_version = false; int verbose = 0; uint64_t batch = 0;
    Arg arg{argc, argv, 2, UPDATE_USAGE};
    for (int& i = arg.i; i < argc; ++i) {
        std::string& a = arg.a;
        a = argv[i]; arg.has_inline = false;
        const size_t eq = a.find('=');
        if (a.rfind("--", 0) == 0 && eq != std::string::npos) { arg.val = a.substr(eq + 1); a = a.substr(0, eq); arg.has_inline = true; }
        int rc = 0;
        if (a == "-h" || a == "--help") { std::fputs(UPDATE_HELP, stdout); return EX_OK_; }
        else if (a == "-d" || a == "--database") rc = arg.need(&database);
        else if (a == "-r" || a == "--reference") rc = arg.need(&reference);
        else if (a == "--hla-gen") rc = arg.need(&gen);
        else if (a == "--hla-nuc") rc = arg.need(&nuc);
        else if (a == "--hla-version") { rc = arg.need(&version); has_version = true; }
        else if (a == "-o" || a == "--output-db") rc = arg.need(&output);
        else if (a == "--batch-alleles") { rc = arg.need_u64(&batch); if (!rc && batch > 0xFFFFFFFFull) rc = clap_error(UPDATE_USAGE, "value too large for '--batch-alleles'"); }
        else if (a == "-v" || a == "--verbose") ++verbose;
        else if (a.size() > 2 && a[0] == '-' && a[1] == 'v' && a.find_first_not_of('v', 1) == std::string::npos) verbose += (int)a.size() - 1;
        else return clap_error(UPDATE_USAGE, "unexpected argument '" + a + "' found");
        if (rc) return rc;
    }
    std::string missing;
    if (database.empty()) missing += "\n  --database <JSON>";
    if (reference.empty()) missing += "\n  --reference <FASTA>";
    if (gen.empty()) missing += "\n  --hla-gen <FASTA>";
    if (nuc.empty()) missing += "\n  --hla-nuc <FASTA>";
    if (output.empty()) missing += "\n  --output-db <JSON>";
    if (!missing.empty()) return clap_error(UPDATE_USAGE, "the following required arguments were not provided:" + missing);
    if (!exists(database)) return noinput("", "Database JSON", database);
    if (!exists(reference)) return noinput("", "Reference FASTA", reference);
    if (!exists(gen)) return noinput("", "HLA genomic FASTA", gen);
    if (!exists(nuc)) return noinput("", "HLA cDNA FASTA", nuc);
    // the host side first: the database, the two FASTA files (DATAERR), the reference
    char err[512];
    sp_database* db = nullptr; sp_hla_alleles* alleles = nullptr; sp_fasta* fasta = nullptr; sp_ctx* ctx = nullptr; sp_hla_config_result* res = nullptr;
    int code = EX_OK_;
    auto done = [&](int c) { sp_hla_config_result_free(res); if (ctx) sp_ctx_destroy(ctx); if (fasta) sp_fasta_free(fasta); sp_hla_alleles_free(alleles); if (db) sp_database_free(db); return c; };
    if (sp_database_load(database.c_str(), &db, err, sizeof err) != SP_OK) { std::fprintf(stderr, "error: Error while loading database: %s\n", err); return done(EX_IOERR_); }
    if (sp_hla_fasta_load(gen.c_str(), nuc.c_str(), &alleles) != SP_OK) { std::fprintf(stderr, "error: Error while reading HLA sequences: %s\n", sp_hla_fasta_last_error()); return done(EX_DATAERR_); }
    sp_hla_alleles_stats st{};
    sp_hla_alleles_info(alleles, &st);
    if (st.warnings && *st.warnings) std::fprintf(stderr, "%s", st.warnings);
    if (sp_fasta_open(reference.c_str(), &fasta, err, sizeof err) != SP_OK) { std::fprintf(stderr, "error: Error while loading reference: %s\n", err); return done(EX_IOERR_); }
    // the device work
    const int32_t crc = sp_ctx_create(0, nullptr, &ctx);
    if (crc != SP_OK) { ctx = nullptr; std::fprintf(stderr, "error: no usable HIP device (sp_ctx_create: status %d)\n", crc); return done(EX_UNAVAILABLE_); }
    const int32_t rc = sp_hla_config_extend(ctx, fasta, db, alleles, (uint32_t)batch, &res);
    if (rc != SP_OK) {
        std::fprintf(stderr, "error: Error while extending HLA coordinates: %s\n", sp_last_error(ctx));
        return done(rc == SP_ERR_HIP || rc == SP_ERR_NO_DEVICE ? EX_UNAVAILABLE_ : EX_DATAERR_);
    }
    uint32_t n_genes = 0, n_alleles = 0; const char* warn = nullptr;
    sp_hla_config_result_info(res, &n_genes, &n_alleles, &warn);
    if (warn && *warn) std::fprintf(stderr, "%s", warn);
    if (verbose) {
        std::fprintf(stderr, "%u alleles (%u with DNA), %u dropped without cDNA, %u of unsupported genes\n", st.n_alleles, st.n_dna, st.n_dropped_no_cdna, st.n_dropped_gene);
        for (uint32_t g = 0; g < n_genes; ++g) {
            sp_hla_cfg_gene x{};
            sp_hla_config_result_gene(res, g, &x);
            std::fprintf(stderr, "%s %s:%llu-%llu%s, %u of %u DNA alleles mapped", x.name, x.chrom, (unsigned long long)x.start, (unsigned long long)x.end, x.moved ? " (updated)" : "", x.n_mapped, x.n_dna_alleles);
            if (x.worst_allele >= 0) {
                const char* id = "";
                sp_hla_alleles_get(alleles, (uint32_t)x.worst_allele, &id, nullptr, nullptr, nullptr, nullptr);
                std::fprintf(stderr, ", worst mapping %s (%d+%d)/%d", id, x.worst_nm, x.worst_unmapped, x.worst_len);
            }
            std::fprintf(stderr, "\n");
        }
    }
    sp_database_metadata md{};
    sp_database_get_metadata(db, &md);
    if (sp_database_save_hla(db, alleles, res, has_version ? version.c_str() : md.hla_version, output.c_str()) != SP_OK) {
        std::fprintf(stderr, "error: Error while writing database: %s\n", sp_database_last_error(db));
        code = EX_IOERR_;
    }
    return done(code);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2 || !std::strcmp(argv[1], "-h") || !std::strcmp(argv[1], "--help")) {
        std::printf("starphase_hip: PGx diplotyping on AMD Instinct GPUs\n\nUsage: starphase_hip <COMMAND> [OPTIONS]\n\nCommands:\n  diplotype        Diplotype a sample from its files\n"
                    "  diplotype-batch  Diplotype the samples of a manifest, many per device pass\n"
                    "  update-hla       Rebuild a database's HLA section from the FASTA files of an IMGT/HLA release\n");
        return argc < 2 ? EX_CLAP : EX_OK_;
    }
    if (!std::strcmp(argv[1], "diplotype-batch")) return batch_main(argc, argv);
    if (!std::strcmp(argv[1], "update-hla")) return update_hla_main(argc, argv);
    if (std::strcmp(argv[1], "diplotype") != 0) return clap_error(USAGE, std::string("unrecognized subcommand '") + argv[1] + "'");
    Options o;
    sp_diplotype_settings& s = o.s;
    sp_diplotype_settings_default(&s);
    const std::string &database = o.database, &reference = o.reference, &include = o.include, &exclude = o.exclude;
    std::string vcf, sv_vcf, output, pharmcat, debug, sample;
    std::vector<std::string> bams;
    const int parsed = parse_options(argc, argv, USAGE, std::string(HELP_HEAD) + HELP_SHARED + HELP_TAIL, o, [&](Arg& arg) -> int {
        const std::string& a = arg.a;
        std::string tmp; uint64_t ignored = 0;
        if (a == "-c" || a == "--vcf") return arg.need(&vcf);
        if (a == "-s" || a == "--sv-vcf") return arg.need(&sv_vcf);
        if (a == "-b" || a == "--bam") { const int rc = arg.need(&tmp); if (!rc) bams.push_back(tmp); return rc; }
        if (a == "-o" || a == "--output-calls") return arg.need(&output);
        if (a == "--pharmcat-tsv") return arg.need(&pharmcat);
        if (a == "--output-debug") return arg.need(&debug);
        if (a == "--sample-name") return arg.need(&sample);
        if (a == "-t" || a == "--threads") return arg.need_u64(&ignored);
        return NOT_MINE;
    });
    if (parsed != PARSED) return parsed;
    std::string missing;
    if (database.empty()) missing += "\n  --database <JSON>";
    if (reference.empty()) missing += "\n  --reference <FASTA>";
    if (output.empty()) missing += "\n  --output-calls <JSON>";
    if (!missing.empty()) return clap_error(USAGE, "the following required arguments were not provided:" + missing);
    // check_diplotype_settings (src/cli/diplotype.rs:200-330): the files first (check_required_filename exits with NOINPUT), then the rules
    if (!exists(database)) return noinput("", "Database JSON", database);
    if (!exists(reference)) return noinput("", "Reference FASTA", reference);
    if (!vcf.empty() && !exists(vcf)) return noinput("", "VCF file", vcf);
    if (!sv_vcf.empty() && !exists(sv_vcf)) return noinput("", "SV VCF file", sv_vcf);
    for (const auto& b : bams) if (!exists(b)) return noinput("", "Alignment file", b);
    std::vector<const char*> bam_ptrs;
    for (const auto& b : bams) bam_ptrs.push_back(b.c_str());
    sp_sample_inputs in{};
    in.n_bams = (uint32_t)bams.size(); in.bams = bam_ptrs.data(); in.vcf = vcf.empty() ? nullptr : vcf.c_str();
    s.include_set = include.empty() ? nullptr : include.c_str(); s.exclude_set = exclude.empty() ? nullptr : exclude.c_str();
    s.sample_name = sample.empty() ? nullptr : sample.c_str(); s.sv_vcf = sv_vcf.empty() ? nullptr : sv_vcf.c_str();
    s.debug_folder = debug.empty() ? nullptr : debug.c_str();
    if (o.debug_reads && debug.empty()) { std::fprintf(stderr, "error: --debug-reads needs a debug folder (--output-debug <DIR>)\n"); return EX_USAGE_; }
    if (o.debug_hla_mappings && debug.empty()) { std::fprintf(stderr, "error: --debug-hla-mappings needs a debug folder (--output-debug <DIR>)\n"); return EX_USAGE_; }
    if (o.debug_hla_ties && debug.empty()) { std::fprintf(stderr, "error: --debug-hla-ties needs a debug folder (--output-debug <DIR>)\n"); return EX_USAGE_; }
    if (o.debug_consensus_support && debug.empty()) { std::fprintf(stderr, "error: --debug-consensus-support needs a debug folder (--output-debug <DIR>)\n"); return EX_USAGE_; }
    if (o.debug_cyp2d6_support && debug.empty()) { std::fprintf(stderr, "error: --debug-cyp2d6-support needs a debug folder (--output-debug <DIR>)\n"); return EX_USAGE_; }
    if (o.debug_cyp2d6_vcf && debug.empty()) { std::fprintf(stderr, "error: --debug-cyp2d6-vcf needs a debug folder (--output-debug <DIR>)\n"); return EX_USAGE_; }
    if (o.debug_cyp2d6_alternatives && debug.empty()) { std::fprintf(stderr, "error: --debug-cyp2d6-alternatives needs a debug folder (--output-debug <DIR>)\n"); return EX_USAGE_; }
    if (o.debug_cyp2d6_alternative_reads && debug.empty()) { std::fprintf(stderr, "error: --debug-cyp2d6-alternative-reads needs a debug folder (--output-debug <DIR>)\n"); return EX_USAGE_; }
    if (o.debug_variant_alternatives && debug.empty()) { std::fprintf(stderr, "error: --debug-variant-alternatives needs a debug folder (--output-debug <DIR>)\n"); return EX_USAGE_; }
    char err[512];
    if (sp_diplotype_settings_check(&s, &in, err, sizeof err) != SP_OK) {
        std::fprintf(stderr, "error: Error while processing CLI settings: %s\n", err);
        return EX_USAGE_;
    }
    if (!include.empty() && !exists(include)) return noinput("", "Include set", include);
    if (!exclude.empty() && !exists(exclude)) return noinput("", "Exclude set", exclude);
    if (!debug.empty() && !make_dirs(debug)) { std::fprintf(stderr, "error: Error while creating debug folder: %s\n", std::strerror(errno)); return EX_IOERR_; }
    // the device work
    int code = EX_OK_;
    sp_starphase* h = create_handle(o, &code);
    if (!h) return code;
    sp_result* result = nullptr;
    const int32_t rc = sp_starphase_call(h, &in, &result);
    const char* warn = sp_starphase_warnings(h);
    if (warn && *warn) std::fprintf(stderr, "%s", warn);
    if (rc != SP_OK) {
        std::fprintf(stderr, "error: Error while calling diplotypes: %s\n", sp_starphase_last_error(h));
        sp_starphase_free(h);
        return EX_DATAERR_;
    }
    if (o.verbose) {
        sp_starphase_timing t{};
        sp_starphase_last_timing(h, &t);
        std::fprintf(stderr, "call %.1f ms (BAM decode %.1f, variant genes %.1f, HLA %.1f with %u reads, CYP2D6 %.1f with %u reads)\n", t.call_ms, t.bam_decode_ms,
                     t.variant_ms, t.hla_ms, t.n_hla_reads, t.cyp_ms, t.n_cyp_reads);
    }
    code = save_result(result, "", output, pharmcat);
    sp_result_free(result);
    sp_starphase_free(h);
    return code;
}

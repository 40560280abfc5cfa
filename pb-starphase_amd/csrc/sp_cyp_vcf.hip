// sp_cyp_vcf.hip -- cyp2d6_alleles.vcf.gz (write_cyp2d6_vcf, src/cyp2d6/vcf_writer.rs), host only: the windows of the database variants on a consensus
// (sp_cyp_variant_windows), the VCF text with the optional read support per variant and region (sp_cyp_alleles_vcf), and a BGZF writer (sp_bgzf_save).
// Contract: include/starphase_hip.h; design: DESIGN.md sections 7.2 and 10.
#include "sp_internal.h"
#include <cstring>
#include <ctime>
#include <string>
#include <vector>
#include <zlib.h>

extern "C" {

// The path of the alignment (query = the consensus, target = the backbone) is followed once per variant: q_lo is the query offset the FIRST time the path has consumed
// the backbone up to lo (in front of an 'I' at that junction), q_hi the query offset the LAST time it has consumed it up to hi (behind such an 'I').
int32_t sp_cyp_variant_windows(const sp_affine_aln* aln, const uint32_t* cigar, uint32_t n_cigar, uint32_t n_variants, const int32_t* var_pos, const uint32_t* var_ref_len,
                               uint32_t flank, sp_window* windows, int32_t* valid) {
    if (!aln || (n_cigar && !cigar) || (n_variants && (!var_pos || !var_ref_len || !windows || !valid))) return SP_ERR_INVALID_ARG;
    for (uint32_t v = 0; v < n_variants; ++v) {
        windows[v] = sp_window{ 0, 0 }; valid[v] = 0;
        const int64_t lo = (int64_t)var_pos[v] - (int64_t)flank, hi = (int64_t)var_pos[v] + (int64_t)var_ref_len[v] + (int64_t)flank;
        if (n_cigar == 0 || lo < (int64_t)aln->b_start || hi > (int64_t)aln->b_end) continue;                // not covered
        int64_t t = aln->b_start, q = aln->a_start, q_lo = -1, q_hi = -1;
        if (t == lo) q_lo = q;
        if (t == hi) q_hi = q;
        for (uint32_t k = 0; k < n_cigar; ++k) {
            const uint32_t op = cigar[k] & 15u; const int64_t n = (int64_t)(cigar[k] >> 4);
            if (op == 1u) q += n;
            else if (op == 7u || op == 8u || op == 2u) {
                const bool on_query = op != 2u;
                if (t < lo && lo <= t + n) q_lo = q + (on_query ? lo - t : 0);
                if (t < hi && hi <= t + n) q_hi = q + (on_query ? hi - t : 0);
                t += n; if (on_query) q += n;
            } else return SP_ERR_INVALID_ARG;
            if (t == hi) q_hi = q;                                                                            // (behind every op that stands at hi: the 'I' ops there included)
        }
        if (t != (int64_t)aln->b_end || q != (int64_t)aln->a_end) return SP_ERR_INVALID_ARG;                  // the ops do not consume the spans
        if (q_lo < 0 || q_hi <= q_lo) continue;                                                               // all of it under one 'D': none
        windows[v] = sp_window{ (uint32_t)q_lo, (uint32_t)q_hi }; valid[v] = 1;
    }
    return SP_OK;
}

int32_t sp_cyp_alleles_vcf(const sp_cyp_db* db, const sp_cyp_call* call, const sp_cyp_region_variants* rv, const sp_window_support* support, const int32_t* support_valid,
                           const char* file_date, const char* command, char* out, uint64_t cap, uint64_t* needed) {
    if (!db || !call || (cap && !out)) return SP_ERR_INVALID_ARG;
    sp_cyp_db_stats st;
    if (sp_cyp_db_info(db, &st) != SP_OK) return SP_ERR_INVALID_ARG;
    const uint32_t NV = st.n_variants;
    std::vector<int32_t> regions;                                             // the sample columns: the typed regions, in region order
    if (call->status == 0 && rv) for (int32_t h = 0; h < call->n_consensus && h < SP_CYP_MAXCONS; ++h) if (rv->has_variants[h] == 1) regions.push_back(h);
    if (!regions.empty() && NV && !rv->state) return SP_ERR_INVALID_ARG;
    char today[16];
    if (!file_date) { const time_t now = time(nullptr); struct tm tm_utc; gmtime_r(&now, &tm_utc); strftime(today, sizeof today, "%Y%m%d", &tm_utc); file_date = today; }
    std::string text = "##fileformat=VCFv4.2\n##FILTER=<ID=PASS,Description=\"All filters passed\">\n";
    text += std::string("##fileDate=") + file_date + "\n##source=starphase_hip\n##reference=GRCh38\n";
    text += std::string("##contig=<ID=") + spi_cyp_db_chrom(db) + ",length=50818468>\n";
    text += "##INFO=<ID=VI,Number=1,Type=String,Description=\"Variant impact\">\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n";
    if (support) {
        text += "##FORMAT=<ID=SR,Number=1,Type=Integer,Description=\"Member reads whose alignment spans the variant's window on the consensus\">\n";
        text += "##FORMAT=<ID=CR,Number=1,Type=Integer,Description=\"Member reads whose alignment spans the variant's window on the consensus and match the consensus at every base of it\">\n";
    }
    text += std::string("##pbstarphase_version=\"\"\n##pbstarphase_command=\"") + (command ? command : "") + "\"\n";
    text += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO";
    if (!regions.empty()) text += "\tFORMAT";
    for (int32_t h : regions) text += "\t" + std::to_string(h) + "_" + spi_cyp_region_label(call, h);
    text += "\n";
    for (uint32_t v = 0; v < NV && !regions.empty(); ++v) {
        bool listed = false;
        for (int32_t h : regions) listed |= rv->state[(size_t)h * NV + v] != 255;
        if (!listed) continue;
        int64_t pos = 0; const char *ref = nullptr, *alt = nullptr, *label = nullptr, *vi = nullptr;
        sp_cyp_db_variant(db, v, &pos, &ref, &alt, &label, nullptr); sp_cyp_db_variant_vi(db, v, &vi);
        text += std::string(spi_cyp_db_chrom(db)) + "\t" + std::to_string(pos + 1) + "\t" + label + "\t" + ref + "\t" + alt + "\t.\t.\t" + (vi ? std::string("VI=") + vi : std::string("."));
        text += support ? "\tGT:SR:CR" : "\tGT";
        for (int32_t h : regions) {
            const uint8_t s = rv->state[(size_t)h * NV + v];
            text += (s == 4 || s == 5) ? "\t." : (s == 1 || s == 2) ? "\t1" : "\t0";                        // Ambiguous* | Match, Unexpected | everything else, 255 included
            if (!support) continue;
            const size_t at = (size_t)h * NV + v;
            if (support_valid && !support_valid[at]) text += ":.:.";
            else text += ":" + std::to_string(support[at].span) + ":" + std::to_string(support[at].exact);
        }
        text += "\n";
    }
    if (needed) *needed = text.size() + 1;
    if (cap < text.size() + 1) { if (cap) out[0] = '\0'; return SP_ERR_CAPACITY; }
    std::memcpy(out, text.c_str(), text.size() + 1);
    return SP_OK;
}

// Standard BGZF: gzip members of up to 65,280 input bytes with the 'BC' extra subfield (BSIZE = the member's size - 1), raw deflate inside, the 28-byte empty member last
int32_t sp_bgzf_save(const char* path, const void* data, uint64_t len) {
    if (!path || (len && !data)) return SP_ERR_INVALID_ARG;
    static const uint8_t eof_marker[28] = { 0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    constexpr uint64_t IN_MAX = 0xff00; constexpr size_t BLOCK_MAX = 65536, HEAD = 18, TAIL = 8;
    FILE* f = std::fopen(path, "wb");
    if (!f) return SP_ERR_INVALID_ARG;
    std::vector<uint8_t> block(BLOCK_MAX);
    const uint8_t* src = (const uint8_t*)data;
    bool ok = true;
    for (uint64_t at = 0; ok && at < len; at += IN_MAX) {
        const uInt n = (uInt)std::min<uint64_t>(IN_MAX, len - at);
        size_t body = 0;
        for (int level : { Z_DEFAULT_COMPRESSION, 0 }) {                       // (input that does not shrink is stored: 65,280 bytes + 5 fit a block)
            z_stream zs; std::memset(&zs, 0, sizeof zs);
            if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) { ok = false; break; }
            zs.next_in = const_cast<Bytef*>(src + at); zs.avail_in = n; zs.next_out = block.data() + HEAD; zs.avail_out = (uInt)(BLOCK_MAX - HEAD - TAIL);
            const int rc = deflate(&zs, Z_FINISH);
            body = zs.total_out;
            deflateEnd(&zs);
            if (rc == Z_STREAM_END) break;
            body = 0;
            if (level == 0) ok = false;
        }
        if (!ok || body == 0) { ok = false; break; }
        const size_t total = HEAD + body + TAIL;
        std::memcpy(block.data(), eof_marker, 16);
        block[16] = (uint8_t)((total - 1) & 0xff); block[17] = (uint8_t)((total - 1) >> 8);
        const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), src + at, n);
        for (int b = 0; b < 4; ++b) { block[HEAD + body + b] = (uint8_t)(crc >> (8 * b)); block[HEAD + body + 4 + b] = (uint8_t)((uint32_t)n >> (8 * b)); }
        ok = std::fwrite(block.data(), 1, total, f) == total;
    }
    ok = ok && std::fwrite(eof_marker, 1, sizeof eof_marker, f) == sizeof eof_marker;
    ok = (std::fclose(f) == 0) && ok;
    return ok ? SP_OK : SP_ERR_INVALID_ARG;
}

int32_t sp_cyp_alleles_vcf_save(const sp_cyp_db* db, const sp_cyp_call* call, const sp_cyp_region_variants* rv, const sp_window_support* support, const int32_t* support_valid,
                                const char* file_date, const char* command, const char* path) {
    if (!path) return SP_ERR_INVALID_ARG;
    char today[16];
    if (!file_date) { const time_t now = time(nullptr); struct tm tm_utc; gmtime_r(&now, &tm_utc); strftime(today, sizeof today, "%Y%m%d", &tm_utc); file_date = today; }      // (one date for both renderings)
    uint64_t need = 0;
    int32_t rc = sp_cyp_alleles_vcf(db, call, rv, support, support_valid, file_date, command, nullptr, 0, &need);
    if (rc != SP_OK && rc != SP_ERR_CAPACITY) return rc;
    std::string text((size_t)need, '\0');
    rc = sp_cyp_alleles_vcf(db, call, rv, support, support_valid, file_date, command, &text[0], need, &need);
    if (rc != SP_OK) return rc;
    return sp_bgzf_save(path, text.data(), need - 1);
}

} // extern "C"

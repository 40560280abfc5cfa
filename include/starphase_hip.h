/*
 * starphase_hip.h -- C ABI of the MI355X (gfx950) StarPhase hot-path library (libstarphase_hip.so).
 *
 * The reference (PacificBiosciences/pb-StarPhase v2.0.1) exposes no FFI of its own for this path; its hot
 * path sits behind ordinary Rust calls whose arithmetic is delegated to minimap2 through
 * minimap2::Aligner::{with_seq,with_index,map}.  The boundary is therefore cut at those call sites
 * (SURVEY.md 8(b)).  Every entry point below names the reference interface it replaces (paths relative
 * to the reference checkout).  INTEGRATION.md shows the Rust `extern "C"` block a maintainer would add.
 *
 * Conventions
 *   - plain C types only; caller owns every host buffer (sizes passed explicitly); the library owns device
 *     memory behind opaque handles; no callbacks.
 *   - every call returns an int32 status (SP_OK = 0); nothing aborts or throws across the boundary;
 *     sp_last_error() returns a NUL-terminated message for the last failing call on that context.
 *   - one sp_ctx = one GPU + one HIP stream; a context is used from one host thread at a time
 *     (the reference is single-threaded: src/cli/diplotype.rs:185-191); contexts are independent.
 *   - calls are stream-ordered and synchronous on return.
 *   - results never depend on launch geometry; ties go to the lowest index in the documented order.
 *   - there is NO CPU fallback: without a usable HIP device sp_ctx_create fails with SP_ERR_NO_DEVICE.
 */
#ifndef STARPHASE_HIP_H
#define STARPHASE_HIP_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SP_ABI_VERSION 2      /* 2 (round 5): sp_hla_realign grew (k1_* fields); the records that grew in round 4 (mm2_* fields of sp_hla_realign, sp_hla_best, sp_region_hit;
                               * sp_cyp_call.searches_gave_up; sp_priority_job.gave_up) are covered by the same step.  A caller checks sp_abi_version() == SP_ABI_VERSION and
                               * sp_struct_size() of every record it allocates before its first call */

/* status codes: "expected" outcomes the reference downgrades (CallerError -> NO_MATCH,
 * src/diplotyper.rs:316-327; src/cyp2d6/errors.rs:4-11) are distinct from fatal ones (src/main.rs:181-185). */
enum {
    SP_OK                  = 0,
    SP_ERR_INVALID_ARG     = 1,
    SP_ERR_NO_DEVICE       = 2,
    SP_ERR_HIP             = 3,
    SP_ERR_OUT_OF_MEMORY   = 4,
    SP_ERR_TOO_LONG        = 5,   /* sequence longer than the kernels support (65,535 bases per window) */
    SP_ERR_CAPACITY        = 6,   /* an output array is too small: call again with more room */
    SP_ERR_CHAIN_COLLAPSE  = 7,   /* the reference panics here ("chain collapse", src/cyp2d6/caller.rs:531-533) */
    SP_ERR_BAD_VARIANT     = 8,   /* NormalizedVariant::new bails (src/data_types/normalized_variant.rs:45-52,66-84,160-168) */
    SP_ERR_NO_CHAINING_HEAD = 16, /* CallerError::NoChainingHead  (src/cyp2d6/chaining.rs:321-323) */
    SP_ERR_NO_CHAINS_FOUND  = 17, /* CallerError::NoChainsFound   (src/cyp2d6/chaining.rs:393-396) */
    SP_ERR_NO_SCORE_PAIRS   = 18  /* CallerError::NoScorePairs    (src/cyp2d6/chaining.rs:559-562) */
};

typedef struct sp_ctx    sp_ctx;
typedef struct sp_seqset sp_seqset;
typedef struct sp_hla_db sp_hla_db;

/* ------------------------------------------------------------------ context */
int32_t sp_abi_version(void);
/* sizeof of a record of this header as THIS build of the library lays it out ("sp_hla_realign", "sp_region_hit", ...; every struct typedef'd here); -1 for an unknown name.
 * A binding checks the records it allocates and the library fills (a record that grew since the binding was generated would overflow the caller's array). */
int32_t sp_struct_size(const char* name);
int32_t sp_device_count(int32_t* count);
/* device: HIP ordinal.  stream: a hipStream_t to run on (e.g. torch's current stream) or NULL to create one. */
int32_t sp_ctx_create(int32_t device, void* stream, sp_ctx** out);
/* What a context found when it was made.  hw_queues: the number of hardware queues the HIP runtime maps this process's streams onto (its GPU_MAX_HW_QUEUES
 * setting; the runtime's own default is 4).  The library runs the loci / genes / samples of a call on streams of their own and wants >= 16: with fewer, two chains
 * of small dependent launches can share a queue with another sample's large grids (measured: 230k instead of 300k reads/s with three samples in flight).  The
 * first sp_ctx_create of a process therefore sets GPU_MAX_HW_QUEUES=16 when the variable is not set (hw_queues_set_by_library = 1) -- which only takes effect
 * if the HIP runtime has not been initialised yet (a host that initialises HIP first should export the variable itself); a value below 16 found in the
 * environment is left alone and reported in `warning` (and once through sp_last_error of that context, status SP_OK). */
typedef struct {
    int32_t device, num_cus;
    int32_t hw_queues;                 /* GPU_MAX_HW_QUEUES as seen at sp_ctx_create (after the library's own default, if it set one) */
    int32_t hw_queues_set_by_library;  /* 1: the variable was not set and the library set it to 16 */
    char warning[256];                 /* "" or what the host should change */
} sp_ctx_info;
int32_t sp_ctx_get_info(const sp_ctx* ctx, sp_ctx_info* out);
void    sp_ctx_destroy(sp_ctx* ctx);
const char* sp_last_error(const sp_ctx* ctx);
int32_t sp_ctx_synchronize(sp_ctx* ctx);
/* Tuning switches of a context.  "hla_split_genes" (default 1): sp_hla_diplotype_genes / sp_hla_diplotype_cohort solve the units of a
 * call (the genes of a sample, the (sample, gene) pairs of a cohort) with >= 1,000 realigned reads side by side on up to
 * "hla_split_streams" (1..4, default 3) streams -- helper streams the context owns, one host thread each for the length of the call:
 * lowest latency for one call; set hla_split_genes to 0 when several samples are in flight on contexts of their own, where the streams
 * of the other samples already fill the gaps (sp_cyp_diplotype follows the same switch: with 1 it places the regions of interest on the consensuses
 * for its weights on a helper stream while it types the consensuses).  The calls are the same either way.  "cons_retry_ladder" (default 0: the reference has no such rule): 1 makes sp_cyp_diplotype* run
 * its multi-way consensus with the retry of searches that give up (sp_cons_config.no_retry_ladder = 0, see sp_consensus_priority); sp_cyp_call.gave_up says whether a search of the call gave up.
 * "k1_best_n" (0..8, default 5 = the reference's `best_n`, src/util/mapping.rs:12): sp_hla_realign_reads maps a read the way realign_record does -- minimizer seeding, chaining and
 * selection of the chains that get a base-level alignment as minimap2's `map-hifi` does them, at most k1_best_n secondary chains per read (sp_hla_seed.hip; statement: oracle/mm2.c
 * omm_hla_k1_seeded) -- and accepts among those mappings only; 0 = the exhaustive search of every allele of every anchored gene (the exact argmin the reference approximates).
 * "mm2_rescore" (default 1): sp_hla_realign_reads, sp_hla_type_consensus / sp_hla_score_consensus and sp_cyp_find_regions also report every mapping they return re-scored
 * the reference's way (fields mm2_*; sp_affine_rescore_batch), and the weights of sp_cyp_weight_segments / sp_cyp_diplotype* are taken from the re-scored placement wherever it is
 * within 16 (edits + unmapped bases) of its segment's smallest; 0 leaves the fields zero, the weights on unit-cost counts, and saves the extra launches; 2 = as 1, but every mapping with edits that do not stand alone
 * takes the DP over all of its rows instead of over the rows around those edits (a check of the shortcut, an order of magnitude slower).
 * "profile_rescore_counts" (default 0): 1 makes every such re-score fetch how many of its mappings it left to the DP (sp_profile_get "<stage>_dp_pairs", e.g. k1_segrs_dp_pairs:
 * launches = re-scores, cells = mappings); the host waits for the device at each one -- for measuring runs.
 * "k8_persistent" (0 | 1 | 2, default 2; also the environment variable SP_K8_PERSISTENT): consensus batches whose problems have at most 1,024 reads each can run as two
 * persistent kernels (step workgroups and one control workgroup per problem on a second stream, resident for the length of the batch; the two sides hand over through one word
 * each in memory: write-through stores, `sc1` loads and memory-side atomics, no L2 fences -- gfx950 behaviour) instead of a launch pair per step -- the
 * same search, bit for bit.  0 never, 1 whenever a batch qualifies, 2 = the library decides: batches of at most eight problems, when the HIP runtime came up with >= 16 hardware
 * queues (a batch's two kernels wait for each other: GPU_MAX_HW_QUEUES, sp_ctx_get_info), LIGHT batches only (at most 64 resident workgroups: a cohort call's late levels, a
 * small sample) and not while single-sample batches ran side by side within the last second; a heavy batch (a single large sample) runs as launch pairs since round 6 -- a launch
 * carries side orders and branching windows, the resident workgroups do not.  The budget of CUs is counted per
 * process (several processes on one device: set 0).  A batch whose control workgroups have not all started within half a second runs as launch pairs instead, by itself (the
 * context then stays away from the mode for 64 batches and says so in sp_ctx_get_info().warning); a search that exceeds the launch-pair loop's own step bound ends the batch
 * with the same error in both modes; no path returns while one of the two kernels is still running.
 * "k8_side_orders" (0..3, default 1; also SP_K8_SIDE_ORDERS) and "k8_compound" (0 | 1, default 1; also SP_K8_COMPOUND): how many work orders a consensus step launch carries
 * per problem beside the search's own -- the window or the expansion another WAITING node of the best-first search will need when its turn comes, made in the same launch
 * (a second row of workgroups); the children of an expansion made ahead wait unseen until the search takes their parent out at that column and are adopted without a launch --
 * and whether a window may be ordered WITH the children of the branch its lookahead votes foresee at its end (taken when the window stands and the exact votes of that column
 * name no other children).  Neither changes what the search does -- strings, read assignment, per-read scores and the number of nodes expanded are those of the one-order search,
 * bit for bit --, only how many dependent launches it takes (a 2,000-read CYP2D6 sample 423 -> 285 launches, the branching sample `*4+*68` / `*1` 2,485 -> 1,417).
 * "k8_side_max_blocks" (default 4096): batches with more step workgroups than this keep to the search's own order.  Persistent batches keep to the search's own order as well.
 * "cyp_cohort_streams" (1..8, default 8): streams sp_cyp_diplotype_cohort spreads its groups of samples over (one host thread each).
 * "k5_block_pairs" (0..1048576, default 4096): sp_cyp_best_chain_pair scores up to this many chain pairs with one workgroup per pair (the few pairs
 * of an ordinary sample: the reads of a pair are shared out over the workgroup), more with one thread per pair; the results are the same.
 * Unknown names: SP_ERR_INVALID_ARG. */
int32_t sp_ctx_set_option(sp_ctx* ctx, const char* name, int64_t value);

/* ------------------------------------------------------------------ sequences
 * Replaces the targets handed to minimap2 via Aligner::with_seq / with_index
 * (src/hla/realigner.rs:56-60,78-79; src/hla/caller.rs:1370-1379; src/cyp2d6/haplotyper.rs:155;
 * src/cyp2d6/chaining.rs:29-30).  bases: concatenated ASCII; offsets[n+1]: start of each sequence.
 * Packed on upload to 2 bits/base + an N plane; anything outside ACGT is 'N' and never matches. */
int32_t sp_seqset_upload(sp_ctx* ctx, const char* bases, const uint64_t* offsets, uint32_t n, sp_seqset** out);
/* The reads of a sample are new for every sample (the read loop of diplotype_hla_batch, src/hla/caller.rs:544-596, and of
 * diplotype_cyp2d6, src/cyp2d6/caller.rs:96-139, hands every record's SEQ to the aligner): their way to the device is part of the
 * path.  An upload stages the caller's bytes through pinned memory in chunks on a copy stream of the context (the copy of chunk k + 1
 * into the staging ring runs under the DMA of chunk k) and packs them on the device.
 *   format SP_SEQ_ASCII    one byte per base (any case; everything but ACGT is 'N'); offsets count bases = bytes
 *          SP_SEQ_BAM4     BAM's SEQ field as stored (SAMv1 4.2: 4 bits per base, high nibble first, "=ACMGRSVTWYHKDBN", each read starting
 *                          on a byte boundary): half the bytes of ASCII over PCIe; offsets[n + 1] count BYTES, lengths[n] bases
 *          SP_SEQ_PACKED2  2 bits per base, four per byte (base b in bits 2 (b & 3) of byte b >> 2, A C G T = 0 1 2 3, no N), each
 *                          sequence starting on a byte boundary: a quarter of the bytes; offsets count BYTES, lengths[n] bases
 * lengths may be NULL for SP_SEQ_ASCII.  A sequence longer than 65,534 bases does not fail the call (one ultra-long read must not cost
 * the sample): it enters the set with length 0, is never aligned, and sp_seqset_skipped counts it.
 * sp_seqset_upload_async returns as soon as the set's tables exist; a worker thread of the library moves the bytes.  The caller's
 * buffers must stay untouched and the set must not be used until sp_seqset_wait has returned SP_OK (it reports what the upload hit).
 * One upload per context is in flight at a time (a second one waits for the first).  While it runs, the context's other calls
 * proceed: the reads of sample i + 1 travel under the kernels of sample i. */
#define SP_SEQ_ASCII   0
#define SP_SEQ_BAM4    1
#define SP_SEQ_PACKED2 2
int32_t sp_seqset_upload_format(sp_ctx* ctx, int32_t format, const void* data, const uint64_t* offsets, const uint32_t* lengths, uint32_t n, sp_seqset** out);
int32_t sp_seqset_upload_async(sp_ctx* ctx, int32_t format, const void* data, const uint64_t* offsets, const uint32_t* lengths, uint32_t n, sp_seqset** out);
int32_t sp_seqset_wait(sp_seqset* set);
int32_t sp_seqset_skipped(const sp_seqset* set, uint32_t* n_skipped);       /* sequences dropped for their length */
void    sp_seqset_free(sp_seqset* set);                                      /* the set's device buffers go back to its context for the next upload (no hipFree, which
                                                                             * would wait for every stream of the device); the context frees them when it is destroyed.
                                                                             * Call it when every call that was given the set has returned */
int32_t sp_seqset_count(const sp_seqset* set, uint32_t* n);
int32_t sp_seqset_length(const sp_seqset* set, uint32_t idx, uint32_t* len);

/* ------------------------------------------------------------------ alignment primitives
 * One cell = one (A, B) pair = one 64-lane wavefront; lane = diagonal.  The alignment contract (banded
 * ends-free edit alignment, deterministic tie rules) is specified in DESIGN.md section 3. */
typedef struct {
    uint32_t a;        /* index into set A (streamed side; minimap2 "query" at most call sites)     */
    uint32_t b;        /* index into set B (window side; minimap2 "target")                          */
    int32_t  diag;     /* anchor diagonal = (b position) - (a position)                              */
    int32_t  max_ed;   /* give up beyond this many edits (0..SP_MAX_ED)                              */
} sp_pair;

typedef struct {
    int32_t ok;        /* 1 = alignment found within max_ed                                          */
    int32_t nm;        /* #X + #I bases + #D bases  (minimap2 Alignment.nm)                          */
    int32_t a_start, a_end;   /* half-open span on A                                                 */
    int32_t b_start, b_end;   /* half-open span on B                                                 */
    int32_t a_len, b_len;
} sp_aln;              /* 32 bytes */

#define SP_BAND    64
#define SP_MAX_ED  511
#define SP_KMER    16
#define SP_NO_DIAG INT32_MIN
/* event word: (type << 30) | b_pos ; b_pos = B bases consumed before the edit */
#define SP_EV_X 0u     /* mismatch                      (cigar 'X', op 8) */
#define SP_EV_D 1u     /* consumes one B base only      (cigar 'D', op 2 when B is the target) */
#define SP_EV_I 2u     /* consumes one A base only      (cigar 'I', op 1 when B is the target) */

/* k-mer vote anchor for each pair (a indexes set A = the k-mer indexed side).  Replaces minimap2's
 * seed+chain stage inside Aligner::map.  diag_out[i] = b_pos - a_pos, votes_out[i] = #votes (0: no anchor). */
int32_t sp_anchor_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B,
                        const uint32_t* a_idx, const uint32_t* b_idx, uint64_t n_pairs,
                        int32_t* diag_out, int32_t* votes_out);

/* Same, up to topk (1..8) placements per pair: peaks of the vote histogram taken best first, every bin within +-128
 * diagonals of a chosen peak cleared before the next one is taken (multi-copy targets, e.g. CYP2D6 and CYP2D7 in one read).
 * diag_out / votes_out hold n_pairs * topk entries; unused slots have votes 0. */
int32_t sp_anchor_batch_topk(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B,
                             const uint32_t* a_idx, const uint32_t* b_idx, uint64_t n_pairs, int32_t topk,
                             int32_t* diag_out, int32_t* votes_out);

/* Align every pair.  Replaces every `aligner.map(...)` on the hot path: src/hla/realigner.rs:116,231,290;
 * src/hla/caller.rs:1277,1436; src/cyp2d6/haplotyper.rs:198,395; src/cyp2d6/chaining.rs:58.
 * events (optional, may be NULL): n_pairs * events_stride words, the first nm of each row are valid. */
int32_t sp_align_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B,
                       const sp_pair* pairs, uint64_t n_pairs,
                       sp_aln* out, uint32_t* events, uint32_t events_stride);

/* Two-piece affine re-score of alignments the library found: the numbers the reference reports.  Every (nm, start, end) of the reference is minimap2's
 * (standard_hifi_aligner, src/util/mapping.rs:8-14: match a = 1 -- 5 in score_read, src/hla/caller.rs:1370-1379 --, mismatch 4, gaps min(6 + 2 l, 26 + l),
 * ambiguous bases -1): the best local alignment through the chain's seeds.  For each pair (a = minimap2's query in set A, b = its target in set B, diag = the
 * diagonal b_pos - a_pos the library's own cell aligned it on) the banded Smith-Waterman optimum under those scores on `band` (64 or 256) diagonals around diag,
 * with the forward decisions and end rules of the restatement's DP (oracle/affine.c is the CPU statement): score, NM = mismatches + gap bases + ambiguous bases,
 * and the half-open spans on both sequences; score 0 = nothing aligns.  On the audited pair classes the numbers equal the minimap2 restatement's
 * (tests/test_oracle_affine.py).  sp_hla_realign_reads, sp_hla_score_consensus / sp_hla_type_consensus, and sp_cyp_find_regions report
 * them beside the library's own counts (fields mm2_*); sp_cyp_weight_segments takes its weights from them near a segment's minimum. */
typedef struct { int32_t a, b, q, e, q2, e2, sc_ambi; } sp_affine_opts;           /* map-hifi: 1, 4, 6, 2, 26, 1, 1 */
typedef struct { int32_t score, nm, a_start, a_end, b_start, b_end; } sp_affine_aln;
int32_t sp_affine_rescore_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_opts* opts,
                                int32_t band, sp_affine_aln* out);
/* The same pairs WITH the alignment itself: out[p] is what sp_affine_rescore_batch writes for the same call, and cigar[p * cigar_stride ..] holds n_cigar[p] ops in
 * BAM encoding (len << 4 | op; 7 '=', 8 'X' -- a column with an ambiguous base is an 'X' --, 1 'I' = bases of the query a only, 2 'D' = bases of the target b only)
 * that cover exactly [b_start, b_end) and [a_start, a_end).  The path is the traceback of the forward pass (oracle/affine.c), not a choice of its own: from the
 * first best cell by anti-diagonal, then row, back through the predecessor the forward pass took in every cell -- H from the diagonal, then E1, F1, E2, F2, each only
 * when strictly greater; a gap continued only where that was strictly better than opening it; F ties to the nearest opening -- to the cell the path started in.  So the
 * ops spell out score, nm and spans of out[p].  n_cigar[p] is the true op count even when it exceeds cigar_stride (the row then holds the first cigar_stride ops,
 * SP_OK: the events_stride convention); score 0 (nothing aligns, or max_ed < 0 = skip) gives n_cigar 0.  The direction records (one byte per cell) live in a
 * scratch of up to 512 MB that the call allocates and frees (a batch runs in chunks of pairs whose rows fit it); the device copies of pairs, results and
 * CIGAR rows (n_pairs * cigar_stride words) are pooled buffers the context keeps, like those of the other batch calls.  A walk that does not arrive in the cell
 * its path started in -- the forward pass's records do not allow it -- fails the call with SP_ERR_HIP instead of returning a path. */
int32_t sp_affine_align_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_opts* opts,
                              int32_t band, sp_affine_aln* out, uint32_t* cigar, uint32_t cigar_stride, uint32_t* n_cigar);

/* ------------------------------------------------------------------ pileup: many alignments -> counts per target column
 * The reduction a person does by eye on a pile of reads under a sequence.  pairs / aln / cigar / cigar_stride / n_cigar are what sp_affine_align_batch (or
 * sp_hla_realign_cigars) returned for the same pairs on the same sets (a = query in A, b = target in B; same encoding, same stride convention).  For target t of B,
 * out[col_offset[t] + j] is column j of t over all pairs that name t (col_offset: n_targets + 1 entries, col_offset[0] = 0 and col_offset[t + 1] - col_offset[t] = the
 * length of t, so out has col_offset[n_targets] entries):
 *   depth  pairs whose alignment has an '=', 'X' or 'D' op on column j        eq / del  the '=' / the 'D' ones of those
 *   x[c]   the 'X' ones whose query base on that column has the 2-bit code c (A C G T = 0 1 2 3) as the packed set holds it: a base outside ACGT is stored with
 *          code 0 (the set's N plane is not consulted), so an 'X' column facing an N of the query counts under x[0]
 *   ins    pairs with an 'I' op between column j and j + 1: one per op, not per base
 * so depth == eq + x[0] + x[1] + x[2] + x[3] + del on every column.  A pair with n_cigar 0 contributes nothing; a target no pair names is all zeros.
 * Every argument is checked on the host before anything is launched or written: an index out of range, spans outside the sequences, ops that do not consume exactly the
 * spans of aln (the rule of sp_affine_cigar_strings; a row cut off at cigar_stride is such a case), an op other than = X I D, a run of length 0, or an 'I' op before the
 * alignment's first target column (no traceback of this library has one) return SP_ERR_INVALID_ARG.
 * Kernel: the pairs are bucketed by target on the host; one workgroup of SP_PILEUP_WAVES waves per (target, tile of SP_PILEUP_TILE columns) keeps the tile's counters in
 * LDS (one plane per field, so the lanes of a run land on different banks); its waves take the target's pairs in turn, 64 ops at a time: a wave-wide prefix sum gives
 * every op its first target column and query base, ops that miss the tile are skipped, the others add to LDS (long runs with the lanes across columns); query bases are
 * read for 'X' ops only; the tile leaves with plain coalesced stores.  No global atomics, and integer counts in any order are exact: the result does not depend on the
 * order of the pairs or on launch geometry.  Device memory: pooled buffers of the context (no allocation on a warm context). */
#define SP_PILEUP_TILE  2048
#define SP_PILEUP_WAVES 4
typedef struct { uint32_t depth, eq, x[4], del, ins; } sp_pileup_col;   /* 32 bytes */
int32_t sp_pileup_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_aln* aln,
                        const uint32_t* cigar, uint32_t cigar_stride, const uint32_t* n_cigar, const uint64_t* col_offset, sp_pileup_col* out);

/* ------------------------------------------------------------------ align + pileup + summary in one device-resident pass
 * sp_affine_align_batch(band = 64, cigar_stride = 4096) followed by sp_pileup_batch and, per target, sp_support_summarize -- without the op rows leaving the device.
 * pairs / opts as sp_affine_align_batch takes them (a = query in A, b = target in B, diag, max_ed < 0: skip), col_offset as sp_pileup_batch takes it.  The band is
 * 64 diagonals; sp_align_pileup_band_batch (below) is the same pass on 256 diagonals, or on 64 with a second try on 256.  Every output is optional (NULL: not computed where nothing else needs it, and never downloaded):
 *   aln        n_pairs records, bit for bit sp_affine_align_batch's
 *   cols       col_offset[n_targets] records, bit for bit sp_pileup_batch's over those alignments (a pair with score 0 contributes nothing)
 *   summaries  one per target of B: what sp_support_summarize returns for the target's columns, with n_aligned = the pairs naming the target with score > 0,
 *              n_unaligned = the other pairs naming it, n_members = n_members[t] when that list is given, n_aligned + n_unaligned otherwise.  A target no pair names
 *              is all zeros but for length (and n_members).
 * How: the alignment is the checkpointed traceback of sp_hla_map_consensus's map kernel (no direction byte per cell), writing compact op rows into one pooled buffer;
 * a pileup kernel of sp_pileup_batch's tile design reads op offsets, op counts and spans from device memory (pairs bucketed by target on the host from `pairs` alone:
 * no op row is walked on the host, the rows are the library's own); a summary kernel makes one pass over each target's columns with a depth histogram of
 * SP_SUPPORT_HIST_BINS bins in LDS -- a target with more pairs than bins is binned coarsely and the median's bin resolved by further passes, never capped.  Integer
 * results, exact in any order.  A batch of more than SP_ALIGN_PILEUP_SLICE pairs runs in slices of that many (in the order given) through one op buffer; a tile that
 * an earlier slice has written is loaded, added to and stored again by its one owner per launch (plain loads and stores, no atomics on global memory).  Device memory:
 * pooled buffers of the context only (a second identical call allocates nothing).
 * Errors: SP_ERR_INVALID_ARG before any launch for a NULL set / col_offset, an index out of range or a col_offset that does not follow B's lengths; SP_ERR_TOO_LONG
 * for sequences the map kernel does not take; SP_ERR_CAPACITY for an alignment of more than 4,096 runs (the row sp_affine_align_batch would have cut off). */
#define SP_ALIGN_PILEUP_SLICE 4096
#define SP_SUPPORT_HIST_BINS  1024
typedef struct { uint32_t n_members, n_aligned, n_unaligned, length, min_depth, median_depth, n_contested, reserved_; } sp_support_summary;   /* 32 bytes; the rule: consensus support, below */
int32_t sp_align_pileup_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_opts* opts,
                              const uint64_t* col_offset, sp_affine_aln* aln, sp_pileup_col* cols, sp_support_summary* summaries, const uint32_t* n_members);

/* The same pass with the band chosen by the caller: sp_align_pileup_batch is this call with band = 64, retry_band = 0, band_used = NULL.
 *   band        64 or 256 diagonals around each pair's diag: aln is bit for bit sp_affine_align_batch's at that band
 *   retry_band  0: none.  256 (with band = 64 only): every pair that was attempted (max_ed >= 0) and came back from the 64-diagonal launch with score 0 or without ops
 *               is aligned again on 256 diagonals, and that result stands -- the rule of sp_hla_consensus_support.  The list of those pairs is made, put in pair order and
 *               read by the second launch on the device: there is no host round trip between the two launches of a slice.
 *   band_used   optional, n_pairs entries: 0 when the pair did not align, otherwise the band (64 or 256) that produced its alignment
 * Any other band / retry_band returns SP_ERR_INVALID_ARG before any launch.  Everything else -- outputs, slices, pooled memory, errors -- as sp_align_pileup_batch.
 * The 256-diagonal launch is the map kernel with four diagonals per lane; it runs its walk's rows again in blocks of SP_ALIGN_PILEUP_WIDE_ROWS target rows (one
 * checkpoint of 3 x 256 scores per block and grid slot). */
#define SP_ALIGN_PILEUP_WIDE_ROWS 128
int32_t sp_align_pileup_band_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_opts* opts,
                                   int32_t band, int32_t retry_band, const uint64_t* col_offset, sp_affine_aln* aln, sp_pileup_col* cols,
                                   sp_support_summary* summaries, const uint32_t* n_members, uint32_t* band_used);

/* ------------------------------------------------------------------ insertion alleles: WHAT the reads insert behind a column
 * sp_pileup_col.ins says how many alignments have an 'I' run behind a column; this list says which bases those runs hold -- what a person reads off the purple marker
 * in IGV.  One record per distinct (target, column, inserted string).  Every 'I' run of an alignment belongs to the column in front of it, the column whose `ins` it
 * counts in; its bases are the query's at the run's query position.
 * Identity of an inserted string is the key (len, p0, p1, h): p0 / p1 hold its first 64 bases as 2-bit codes (A C G T = 0 1 2 3), base i in bits [2 i, 2 i + 1] of p0
 * for i < 32 and in bits [2 (i - 32), 2 (i - 32) + 1] of p1 for 32 <= i < 64, zero padded; h is the 64-bit FNV-1a (offset basis 0xcbf29ce484222325, prime
 * 0x100000001b3) over the 2-bit codes of all len bases, one code per step.  Up to 64 bases the key is the string; beyond, the key is the definition of "the same
 * insertion" (two longer strings with one key are one record).  A run that holds a base outside ACGT (the query set's N plane) is not listed: it counts in n_other.
 *   col         the column in the caller's col_offset space (col_offset[t] + j for column j of target t)
 *   count       alignments that carry the string behind the column
 *   first_pair  the lowest pair index among them; first_qpos the run's position in that pair's query -- where a caller fetches a string of more than 64 bases
 *   n_other     on the first record of a column: the column's runs that are not listed (a base outside ACGT), 0 on the others.  A column whose runs are all of that
 *               kind has one record with len = 0, count = 0 (p0 = p1 = h = first_pair = first_qpos = 0)
 * so count + n_other summed over a column's records is the column's sp_pileup_col.ins.  Order: col ascending, then count descending, len ascending, (p0, p1, h)
 * ascending (a record with len 0 has no neighbour in its column).  The list does not depend on the order of the pairs or on launch geometry.
 * Kernels: one wave per alignment lists its runs (key, pair, query position) into a pooled buffer; the runs are binned by (target, tile of
 * SP_PILEUP_TILE columns); one workgroup per tile sorts its runs on the whole key (a bitonic network in LDS; a tile with more than SP_PILEUP_INS_LDS_RUNS runs sorts in
 * its slice of the pooled buffer instead, same code, same result), run-length compacts them, sorts the records into the order above and writes them to its slice of a
 * pooled output; a last pass packs the slices.  Atomics: the sums (run cursor, runs per tile) do not depend on their order; the PLACES a run takes in the run buffer
 * and in its tile's slice do -- the list does not, because the sort that follows is on a total order ((pair, qpos) is unique, and the runs with a base outside ACGT
 * are made identical), so every arrival order sorts to the same sequence.
 * Pooled buffers only; the run buffer is guessed at four runs per pair plus one per 64 query bases, and a batch with more makes the WHOLE pass run once more on a
 * buffer that holds them (a warm context does not).
 * sp_pileup_ins_batch: the list over host op rows -- arguments and checks of sp_pileup_batch.  sp_align_pileup_ins_batch: sp_align_pileup_band_batch that also lists
 * the insertions of the alignments it piles up; ins == NULL is that call, nothing else is launched and no further pool memory is taken.
 * ins holds ins_cap records; *n_ins = the number there are; SP_ERR_CAPACITY when n_ins > ins_cap (every other output is complete, ins is not written: call again with
 * more room).  n_ins must be given with ins. */
#define SP_PILEUP_INS_LDS_RUNS 1024
typedef struct {
    uint64_t col;
    uint32_t len, count;
    uint64_t p0, p1, h;
    uint32_t first_pair, first_qpos;
    uint32_t n_other, reserved_;
} sp_pileup_ins;   /* 56 bytes */
int32_t sp_pileup_ins_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_aln* aln,
                            const uint32_t* cigar, uint32_t cigar_stride, const uint32_t* n_cigar, const uint64_t* col_offset,
                            sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins);
int32_t sp_align_pileup_ins_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_opts* opts,
                                  int32_t band, int32_t retry_band, const uint64_t* col_offset, sp_affine_aln* aln, sp_pileup_col* cols,
                                  sp_support_summary* summaries, const uint32_t* n_members, uint32_t* band_used,
                                  sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins);
/* The ASCII of a record (host only).  Up to 64 bases it comes from the key; a longer string is read from sequence `query` of `queries` at rec->first_qpos -- the query
 * of pair rec->first_pair of the call that made the record (pairs[first_pair].a); both may be NULL / 0 for a record of up to 64 bases, SP_ERR_INVALID_ARG for a longer one
 * without them or with a position outside the sequence.  out / cap / needed as sp_cyp_alleles_json (NUL-terminated; *needed = len + 1; SP_ERR_CAPACITY).
 * NOT directly on the records of the HLA / CYP2D6 support calls when len > 64: there first_pair names a read (or a mapping record) and first_qpos is a position in the
 * member's SEGMENT, which the caller's read set does not hold as a sequence.  CYP2D6: the string is read r = mappings[first_pair].read at
 * [mappings[first_pair].read_start + first_qpos, + len).  HLA, forward gene: read first_pair at [seg_start + first_qpos, + len); reverse gene: the reverse complement
 * of read first_pair at [seg_end - first_qpos - len, seg_end - first_qpos).  (Up to 64 bases the key is the string and none of this is needed; the support calls
 * align on 64 diagonals, where a run of more than 64 bases does not fit -- only the HLA pass's second try on 256 can list one.) */
int32_t sp_support_ins_string(const sp_pileup_ins* rec, const sp_seqset* queries, uint32_t query, char* out, uint64_t cap, uint64_t* needed);

/* ------------------------------------------------------------------ read haplotypes: WHICH reads disagree together at the contested columns
 * The counts of two contested columns cannot say whether their mismatches sit in the same reads (two haplotypes collapsed into one consensus) or are scattered over
 * the reads (noise).  This list can: it is the pile sorted by the reads' calls at the contested columns, what a person does in IGV with "sort by base".
 * Columns used: for target t, c_0 < c_1 < ... < c_{K'-1} are its contested columns by the rule of sp_support_contested over the FINISHED table (all pairs of the batch,
 * all slices); the first K = min(K', SP_SUPPORT_HAP_COLS) of them are used.  K' is reported (n_cols_total), so a cut is visible.
 * The call of an aligned pair (n_cigar > 0; in sp_align_pileup_hap_batch also score > 0 -- the pairs the table counts) at column j of its target is a 4-bit code:
 *   low 3 bits  0 the alignment does not cover j (j outside [b_start, b_end));  1 an '=' op;  2 + c an 'X' op whose query base has the 2-bit code c, exactly as
 *               sp_pileup_col.x[c] counts it (a base outside ACGT is code 0: call 2);  6 a 'D' op
 *   bit 3       set when an 'I' run of that alignment sits directly behind column j -- the run that sp_pileup_col.ins of j counts
 * The pattern of a pair is its K calls packed into w[4]: call k in bits [4 (k mod 16), 4 (k mod 16) + 4) of w[k / 16]; unused bits are zero.
 * One sp_support_hap record per distinct (target, pattern) over the aligned pairs that name the target:
 *   target      the target (in the support calls: the slot of the caller's col_offset)      n_cols   K
 *   count       aligned pairs with this pattern                                              first_pair  the lowest pair index among them
 * Order: target ascending, then count descending, then the 256-bit pattern ascending with w[3] most significant.  A target with K' = 0, or with no aligned pair, has
 * no records.  One sp_support_hap_head per target: its records are haps[first_record .. first_record + n_records), n_cols = K, n_cols_total = K'.
 * Invariants: for a target with K > 0 the counts of its records sum to the aligned pairs naming it (n_aligned of its summary) -- the all-zero pattern of the pairs that
 * span none of the columns is a record like any other; for every used column c_k the counts summed over the records whose call k has low bits 1 / 2 + c / 6 equal that
 * column's eq / x[c] / del, and over the records with bit 3 set its ins.  The list does not depend on the order of the pairs or on launch geometry, except that
 * first_pair follows the caller's indices.
 * Kernels: one workgroup per target lists the first SP_SUPPORT_HAP_COLS contested columns of the finished table (on the device: no host round
 * trip between pileup, list and patterns); one wave per aligned pair stages its target's list in LDS, walks its op row 64 ops at a time (the prefix sums of the pileup
 * kernel), finds the listed columns inside each op's run by binary search and ORs the calls into the pair's pattern in LDS (a column is covered by at most one non-'I'
 * op of an alignment, so the order of the ORs cannot matter); query bases are read for 'X' ops only; the pattern leaves with a plain store.  One workgroup per target
 * then sorts its (pattern, pair) keys on that total order -- a bitonic network in LDS; a target with more than SP_SUPPORT_HAP_LDS_KEYS pairs sorts in its slice of a
 * pooled buffer, same code, same result --, run-length compacts them, sorts the records into the order above; a pack pass writes the list and the heads.  No global
 * atomics.  Pooled buffers only.
 * sp_pileup_hap_batch: the list over host op rows -- arguments and checks of sp_pileup_batch.  sp_align_pileup_hap_batch: sp_align_pileup_ins_batch that also makes this
 * list; haps == NULL is that call, nothing else is launched and no further pool memory is taken.  With haps, a batch of more than SP_ALIGN_PILEUP_SLICE pairs keeps
 * the op rows of every slice (the contested set is known only after the last one): the op buffer then holds the batch's rows, nothing is aligned twice.
 * haps holds hap_cap records; *n_haps = the number there are; heads: one per target of B.  SP_ERR_CAPACITY when n_haps > hap_cap: every other output is complete, haps
 * and heads are not written.  n_haps and heads must be given with haps. */
#define SP_SUPPORT_HAP_COLS     64
#define SP_SUPPORT_HAP_LDS_KEYS 1024
typedef struct {
    uint64_t target;
    uint32_t n_cols, count;
    uint32_t first_pair, reserved_;
    uint64_t w[4];
} sp_support_hap;        /* 56 bytes */
typedef struct {
    uint64_t first_record;
    uint32_t n_records, n_cols;
    uint32_t n_cols_total, reserved_;
} sp_support_hap_head;   /* 24 bytes */
int32_t sp_pileup_hap_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_aln* aln,
                            const uint32_t* cigar, uint32_t cigar_stride, const uint32_t* n_cigar, const uint64_t* col_offset,
                            sp_support_hap* haps, uint64_t hap_cap, uint64_t* n_haps, sp_support_hap_head* heads);
int32_t sp_align_pileup_hap_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_opts* opts,
                                  int32_t band, int32_t retry_band, const uint64_t* col_offset, sp_affine_aln* aln, sp_pileup_col* cols,
                                  sp_support_summary* summaries, const uint32_t* n_members, uint32_t* band_used,
                                  sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins,
                                  sp_support_hap* haps, uint64_t hap_cap, uint64_t* n_haps, sp_support_hap_head* heads);
/* A pattern as text (host only): one token per used column -- '=' a match, 'A' 'C' 'G' 'T' a mismatch with that base, '-' a deletion, '?' not covered -- each followed
 * by '+' when bit 3 is set (a low code of 7 is written '?').  out / cap / needed as sp_support_ins_string; SP_ERR_INVALID_ARG for n_cols > SP_SUPPORT_HAP_COLS. */
int32_t sp_support_hap_string(const sp_support_hap* rec, char* out, uint64_t cap, uint64_t* needed);

/* ------------------------------------------------------------------ window support: HOW MANY reads agree with the target over a whole interval
 * The column table cannot say whether the reads that disagree at column j and at column j + 3 are the same reads; a count per INTERVAL can.  A window is a half-open
 * interval [start, end) of target columns, start < end <= the target's length.  Target t owns windows[win_offset[t] .. win_offset[t + 1]) (win_offset: n_targets + 1
 * entries, win_offset[0] = 0, ascending); inside a target they come in any order and may overlap, nest or repeat.  out[win_offset[t] + i] counts, over the aligned pairs
 * that name t (n_cigar > 0; in sp_align_pileup_windows_batch also score > 0 -- the pairs the table counts), with [b_start, b_end) the pair's target span:
 *   span     b_start <= start && end <= b_end
 *   partial  the two intervals intersect, but the pair does not span the window
 *   exact    the pair spans the window, every column of it lies under an '=' op, and no 'I' op sits at an INTERIOR junction of it: an 'I' between columns j and j + 1
 *            counts when start <= j && j + 1 < end.  Insertions at the two outer junctions do not count, on either side (the rule is symmetric on purpose)
 * reserved_ is 0.  A target without pairs, or a pair that did not align, contributes zeros.  exact <= span, and span + partial <= the pairs naming the target.
 * Kernel: one workgroup of SP_WINDOW_WAVES waves per (target, chunk of SP_WINDOW_CHUNK windows); every lane keeps SP_WINDOW_CHUNK / 64 windows
 * and their three counters in registers.  The waves take the target's pairs in turn; a pair that spans none of the wave's windows is not walked; otherwise the wave
 * walks the op row ONCE, 64 ops at a time (the prefix sums of the pileup kernel), and compacts the pair's defects -- runs of columns under 'X' or 'D', junctions with an
 * 'I' -- into LDS, in doubled coordinates (column c = [2 c, 2 c + 1), junction behind column j = [2 j + 1, 2 j + 2)), where they are sorted and disjoint by construction;
 * each lane then decides its windows by a binary search.  A pair with more than SP_WINDOW_DEFECTS - 64 defects is decided in several such rounds (a window is inexact
 * when any round finds a defect in it).  The waves' counters meet in LDS at the end; one thread per window stores its record.  No atomics at all; integer counts, exact
 * in any order of the pairs and for any launch geometry.  Pooled buffers only.
 * sp_pileup_windows_batch: over host op rows -- arguments and checks of sp_pileup_batch, and SP_ERR_INVALID_ARG before any launch for a window with start >= end or end
 * beyond its target, or a win_offset that does not start at 0 and ascend.
 * sp_align_pileup_windows_batch: sp_align_pileup_band_batch that also counts the windows from the op rows in the pooled op buffer (same checks of the windows);
 * windows == NULL is exactly that call: nothing more is launched or pooled.  A batch of more than SP_ALIGN_PILEUP_SLICE pairs accumulates across slices as the column
 * tiles do: a chunk's workgroup is the one owner of its records in its launch and loads, adds to and stores them (plain loads and stores). */
#define SP_WINDOW_CHUNK   256
#define SP_WINDOW_WAVES   4
#define SP_WINDOW_DEFECTS 256
typedef struct { uint32_t start, end; } sp_window;
typedef struct { uint32_t span, exact, partial, reserved_; } sp_window_support;   /* 16 bytes */
int32_t sp_pileup_windows_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_aln* aln,
                                const uint32_t* cigar, uint32_t cigar_stride, const uint32_t* n_cigar, const uint64_t* col_offset,
                                const uint64_t* win_offset, const sp_window* windows, sp_window_support* out);
int32_t sp_align_pileup_windows_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_opts* opts,
                                      int32_t band, int32_t retry_band, const uint64_t* col_offset, sp_affine_aln* aln, sp_pileup_col* cols,
                                      sp_support_summary* summaries, const uint32_t* n_members, uint32_t* band_used,
                                      const uint64_t* win_offset, const sp_window* windows, sp_window_support* win_out);

/* ------------------------------------------------------------------ HLA database
 * Replaces HlaRealigner::new + create_hla_fasta (src/hla/realigner.rs:42-91,497-526) and the per-call
 * one-sequence indexes of score_read (src/hla/caller.rs:1370-1379).
 * Alleles must be given in database key order ("HLA:HLA00001" ascending = BTreeMap order,
 * src/hla/caller.rs:1413) because ties go to the lowest index.
 *   gene_of[i]      gene index of allele i
 *   dna / cdna      gene-strand sequences as stored in the database (dna length 0 = no DNA sequence)
 *   gene_ref        hg38-forward reference sequence of each gene region incl. the +-100 bp buffer
 *                   (src/hla/realigner.rs:74-81)
 *   gene_fwd[g]     is_forward_strand
 *   exon_start/end  exon coordinates of gene g relative to gene_ref[g] start (hg38 order),
 *                   exon_off[g]..exon_off[g+1]  
 */
typedef struct {
    uint32_t n_alleles, n_genes;
    const uint32_t* gene_of;
    const char* dna;   const uint64_t* dna_off;     /* n_alleles+1 */
    const char* cdna;  const uint64_t* cdna_off;    /* n_alleles+1 */
    const char* gene_ref; const uint64_t* gene_ref_off;   /* n_genes+1 */
    const uint8_t* gene_fwd;
    const uint32_t* exon_off;                        /* n_genes+1 */
    const int32_t* exon_start; const int32_t* exon_end;
    int32_t ref_buffer;                              /* bases of buffer on each side of the gene inside gene_ref (100) */
} sp_hla_db_desc;

int32_t sp_hla_db_create(sp_ctx* ctx, const sp_hla_db_desc* desc, sp_hla_db** out);
void    sp_hla_db_free(sp_hla_db* db);

/* ------------------------------------------------------------------ K1: read -> best database allele
 * Replaces HlaRealigner::realign_record (src/hla/realigner.rs:98-350) for a batch of reads.
 * reads: hg38-forward read sequences already on the device. For read r:
 *   best_allele  index of the accepted allele (lowest nm/(target_len-unmapped) subject to the 0.5 / 0.03
 *                cut-offs, :137-141) or -1;  gene = gene_of[best_allele]
 *   aln          alignment of the read (B) against that allele in hg38 orientation (A): bm.query_* = b_*,
 *                bm.target_* = a_*
 *   seg_start/end  optimal_segment_start..end on the read (:266-267), dna_offset / hpc_offset (:270-325);
 *                status 0 = realigned, 1 = no acceptable allele, 2 = best mapping not Forward (:178-193), 3 = segment failed to map to the gene reference.
 * Seeded mode (context option "k1_best_n" > 0, the default): the mappings a read is judged on are the ones minimap2 would return -- (19,19)-minimizer seeds through the occurrence
 * filter, chains per (strand, allele), the primary chains and the k1_best_n best secondaries within 0.8 of their primary -- base-aligned by the library's cell (64 diagonals around the
 * chain, 256 when that finds nothing) and re-scored with the two-piece affine scores; the acceptance loop runs over them in minimap2's output order on the re-scored numbers
 * (aln = the accepted mapping's cell, mm2_* = its re-score); status 2 = the accepted mapping is on the reverse strand.  k1_chains / k1_mappings / k1_chain_score: chains found for
 * the read, mappings that came back, chain score of the accepted one.  Exhaustive mode ("k1_best_n" = 0; always when cell_out is given): every allele of every gene the read anchors
 * in (>= 16 16-mer votes and >= 1/10 of the best gene's) is a cell, the lowest index wins ties, the counts are the unit-cost ones and mm2_* a report beside them; status 2 is decided at the
 * seeds (the read's best anchor on the reverse-complemented gene references has more 16-mer votes than its best forward anchor -- only reads with fewer than 512 forward votes are
 * anchored a second time, and a read that realigned acceptably forwards is only dropped when the reverse anchor has at least twice the votes; the other fields then hold what the
 * forward search found); k1_* are 0.
 */
typedef struct {
    int32_t status;
    int32_t best_allele;
    int32_t gene;
    int32_t nm, target_len, unmapped;         /* MappingStats of the best allele (:132-133) */
    sp_aln  aln;
    int32_t seg_start, seg_end;
    int32_t dna_offset, hpc_offset;
    /* the same mapping re-scored the reference's way (two-piece affine gaps, end clipping: sp_affine_rescore_batch on the 64 diagonals around aln): what minimap2
     * reports for this read and allele -- NM, the allele span (target_start / target_end), the read span (query_start / query_end); mm2_score 0 = not re-scored
     * (no best allele).  Exhaustive mode: a report beside the counts above, which decide; left zero with context option "mm2_rescore" 0.
     * Seeded mode: these ARE the numbers the acceptance loop ran on (<= 0.03 edit fraction, <= 0.5 penalised: mm2_nm over the re-scored extent) and they are written whatever
     * "mm2_rescore" says; nm / unmapped / aln above stay the unit-cost cell's numbers of the same mapping, so a record judged by nm / target_len alone may look as if it
     * missed or passed a cut-off it did not.  status 2 in seeded mode: best_allele is -1 and mm2_* are 0; sp_hla_realign_seeded_audit hands out the reverse-strand mapping that was accepted
     * (its allele, t_len, nm and spans). */
    int32_t mm2_score, mm2_nm;
    int32_t mm2_t_start, mm2_t_end, mm2_q_start, mm2_q_end;
    int32_t k1_chains, k1_mappings, k1_chain_score;      /* seeded mode: chains of the read, mappings returned, chain score of the accepted mapping */
    int32_t reserved_;
} sp_hla_realign;

/* what the seeded map of a read came to (the audit entry point below; sp_hla_realign carries the same counts) */
#define SP_K1_SEL 16                      /* selected chains per read that are base-aligned (primaries + k1_best_n secondaries; the best ranked when a read has more) */
typedef struct { int32_t n_chains, n_selected, n_mappings, pick, chain_score, rev; } sp_k1_seed_info;
typedef struct {
    int32_t allele, rev, chain_score, n_seeds, t_len;
    int32_t sel_rank;                        /* position among the selected chains */
    int32_t diag;                            /* the cell's diagonal: read position - allele position, midway between the chain's outermost seeds */
    int32_t ok, cell_nm, a_start, a_end, b_start, b_end;   /* the unit-cost cell: A = allele, B = read on the mapped strand */
    int32_t dp_max, nm, t_start, t_end, q_start, q_end;    /* the re-scored mapping (read in forward coordinates, as minimap2 reports) */
    int32_t primary;
} sp_k1_seed_hit;
/* Audit of the seeded stage (tests hold every stage to oracle/mm2.c):
 *   sp_hla_seed_index_info   out[4] = minimizers in the index of the database's DNA alleles, distinct minimizers, the occurrence threshold mid_occ, indexed alleles (built on first use)
 *   sp_seqset_sketch         the (19,19)-minimizers of sequence idx of a set in position order: hash, end position of the k-mer, strand of the smaller k-mer; *n_out may exceed cap
 *   sp_hla_realign_seeded_audit  for read `read` of the set: its chains in rank order (chains[i*10..] = {indexed allele number, rev, chain score, seeds, query start, query end (forward
 *                            coordinates), target start, target end, -, selected}), its mappings in output order (hits, SP_K1_SEL entries), the accepted one (*pick or -1) and
 *                            counters[4] = {kept seeds, anchors, largest anchor count of a read, reads that hit a capacity} of the whole batch */
int32_t sp_hla_seed_index_info(sp_ctx* ctx, const sp_hla_db* db, int64_t* out /* 4 */);
int32_t sp_seqset_sketch(sp_ctx* ctx, const sp_seqset* set, uint32_t idx, uint64_t* hash, int32_t* end_pos, uint8_t* strand, uint32_t cap, uint32_t* n_out);
int32_t sp_hla_realign_seeded_audit(sp_ctx* ctx, const sp_hla_db* db, const sp_seqset* reads, uint32_t read, int32_t* chains, uint32_t chain_cap, uint32_t* n_chains,
                                    sp_k1_seed_hit* hits /* SP_K1_SEL */, uint32_t* n_hits, int32_t* pick, uint64_t* counters /* 4 */);
/* Audit of the re-score of mappings the library holds (the mm2_* numbers and K1's second-stage extents; tests hold every route of it to oracle/affine.c):
 *   sp_affine_rescore_mappings_audit  for each pair (a in set A = the streamed side, b in set B = the window side, diag and max_ed as sp_align_batch takes them;
 *                            max_ed < 0 = no mapping) the pair's cell is run as sp_align_batch runs it -- the alignment "the caller holds" -- and re-scored the way
 *                            the library's own callers have it re-scored, with exactly these knobs: band (64 | 256 diagonals of the DP), target_is_a (which set is
 *                            minimap2's target), events_stride (edit events kept per pair, 1 .. SP_MAX_ED + 1: a mapping with more takes the DP over all rows),
 *                            windows (1: the DP runs over the rows around the clustered edits, context option "mm2_rescore" 1; 0: over all rows, option 2),
 *                            ends_only (0: all six numbers; > 0: the caller takes the extent only, K1's second stage passes 64).  out[p] as
 *                            sp_affine_rescore_batch reports (a_* on the query, b_* on the target); route[p] = 0 closed form (no DP), 1 DP over the rows around
 *                            the clusters, 2 DP over all rows, 3 no mapping; diag[p] = the diagonal, target position - query position, the DP is (or would be)
 *                            centred on: the middle diagonal of the cell's alignment, the cell's own when the cell found none */
int32_t sp_affine_rescore_mappings_audit(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_opts* opts,
                                         int32_t band, int32_t target_is_a, uint32_t events_stride, int32_t windows, int32_t ends_only, sp_affine_aln* out,
                                         int32_t* route, int32_t* diag);

int32_t sp_hla_realign_reads(sp_ctx* ctx, const sp_hla_db* db, const sp_seqset* reads,
                             sp_hla_realign* out /* n_reads */,
                             uint32_t* cell_out /* optional n_reads*n_alleles: (nm<<16 | span) or 0xFFFFFFFF */);
/* sp_hla_realign_reads in seeded mode (k1_best_n > 0, else SP_ERR_INVALID_ARG) that also names every read it drops on the reverse strand: out[] is what
 * sp_hla_realign_reads writes for the same set; rev[r] is, for a record with status 2 and best_allele -1, the accepted reverse-strand mapping of
 * realign_record's loop (src/hla/realigner.rs:124-146,178-193: penalty <= 0.5, edit fraction <= 0.03, the lowest edit fraction wins) -- the indexed
 * allele, its length, NM and the target span (unmapped = t_len - (t_end - t_start)); allele -1 for every other read.  It comes out of the same launches
 * as the records (the pick stage writes it), so it costs no per-read audit. */
typedef struct { int32_t allele, t_len, nm, t_start, t_end, reserved_; } sp_hla_rev_hit;
int32_t sp_hla_realign_reads_rev(sp_ctx* ctx, const sp_hla_db* db, const sp_seqset* reads, sp_hla_realign* out /* n_reads */, sp_hla_rev_hit* rev /* n_reads */);
/* HOW the accepted reads align: for every record with status 0 the CIGAR (sp_affine_align_batch's encoding and stride convention) of the read (query) against
 * best_allele in hg38 orientation (target) at the map-hifi scores {1, 4, 6, 2, 26, 1, 1} -- the alignment whose numbers the record's mm2_* fields are: it covers
 * mm2_t_start..mm2_t_end and mm2_q_start..mm2_q_end, and its X + I + D bases are mm2_nm.  Other records get n_cigar 0.  The band (64 diagonals, 256 for an alignment
 * across a long gap) and the diagonal are derived from the record's own cell (aln) the way the re-score derived them; a pair whose traceback does not reproduce the
 * record is run on the other band, and one that matches on neither is an error (SP_ERR_INVALID_ARG: the records are not this read set's). */
int32_t sp_hla_realign_cigars(sp_ctx* ctx, const sp_hla_db* db, const sp_seqset* reads, const sp_hla_realign* records, uint32_t n_reads,
                              uint32_t* cigar, uint32_t cigar_stride, uint32_t* n_cigar);

/* ------------------------------------------------------------------ K2: consensus -> every allele of a gene
 * Replaces score_read's allele loop + HlaProcessedMatch (src/hla/caller.rs:1411-1510,
 * src/hla/processed_match.rs:53-263).  cons_dna / cons_cdna: gene-strand consensus and its spliced cDNA
 * (ASCII).  require_dna mirrors --hla-require-dna, disable_cdna mirrors --disable-cdna-scoring.
 *   best_allele  running-best winner in database order, -1 if nothing maps (best id stays empty, :1503-1509)
 *   stats        optional n_alleles*6: cdna (len, nm, unmapped), dna (len, nm, unmapped); -1,-1,-1 = None;
 *                rows of alleles of other genes are left at -2.
 */
typedef struct {
    int32_t best_allele;
    int32_t n_scored;            /* alleles visited (gene match and allowed) */
    /* HlaMappingStats of the best allele re-scored the reference's way (a = 5, two-piece affine gaps: sp_affine_rescore_batch): cDNA (len, nm, unmapped), DNA (len, nm,
     * unmapped); -1, -1, -1 = level absent or not re-scored (context option "mm2_rescore" 0).  The running-best scan itself uses the library's own counts. */
    int32_t mm2_stats[6];
} sp_hla_best;

int32_t sp_hla_score_consensus(sp_ctx* ctx, const sp_hla_db* db, uint32_t gene,
                               const char* cons_dna, uint32_t cons_dna_len,
                               const char* cons_cdna, uint32_t cons_cdna_len,
                               int32_t require_dna, int32_t disable_cdna,
                               sp_hla_best* best, int32_t* stats);

/* the same for n consensuses at once (different genes allowed): every (consensus, allele) pair of a level is one cell of one launch,
 * one scan workgroup per consensus.  No per-allele statistics in the batched form. */
int32_t sp_hla_score_consensus_batch(sp_ctx* ctx, const sp_hla_db* db, uint32_t n, const uint32_t* genes,
                                     const char* const* cons_dna, const uint32_t* cons_dna_len,
                                     const char* const* cons_cdna, const uint32_t* cons_cdna_len,
                                     int32_t require_dna, int32_t disable_cdna, sp_hla_best* best /* n */);

/* Replaces score_consensus (src/hla/caller.rs:1258-1319) + splice_read (:1518-1576): the hg38-forward consensus is
 * placed on the un-buffered gene reference (GPU alignment with traceback), its exon bases are spliced out through the
 * aligned pairs, both sequences are put on the gene strand and handed to the K2 scoring above.
 * An empty consensus or one that does not align to the reference gives best_allele = -1 and n_scored = 0
 * (caller.rs:1263-1267,1282-1287).  cdna_out (optional, cdna_cap bytes) receives the spliced gene-strand cDNA. */
int32_t sp_hla_type_consensus(sp_ctx* ctx, const sp_hla_db* db, uint32_t gene,
                              const char* consensus_fwd, uint32_t consensus_len,
                              int32_t require_dna, int32_t disable_cdna,
                              sp_hla_best* best, int32_t* stats,
                              char* cdna_out, uint32_t cdna_cap, uint32_t* cdna_len);

/* n hg38-forward consensuses at once: one placement launch, host splicing, one batched K2 (the gene drivers type all the
 * consensuses of a sample / cohort this way). */
int32_t sp_hla_type_consensus_batch(sp_ctx* ctx, const sp_hla_db* db, uint32_t n, const uint32_t* genes,
                                    const char* const* consensus_fwd, const uint32_t* consensus_len,
                                    int32_t require_dna, int32_t disable_cdna, sp_hla_best* best /* n */);

/* ------------------------------------------------------------------ K2 map: score_read's per-allele mappings
 * score_read (src/hla/caller.rs:1332-1511) also returns the cDNA and DNA mapping of the consensus against EVERY allowed allele of its gene (ReadMappingStats, written to
 * hla_debug.json, src/hla/debug.rs:64-183).  sp_hla_map_consensus(_batch) take the arguments of sp_hla_score_consensus(_batch), run the same K2 and then, for every
 * (consensus, level, allowed allele) whose own cell found an alignment, the two-piece affine alignment at {5, 4, 6, 2, 26, 1, 1} on the 64 diagonals around that cell's
 * diagonal ((b_start - a_start + b_end - a_end) / 2 of the cell): the pair, diagonal and band of the winner's mm2_stats.  For the same pair, diagonal, band and scores
 * the sp_affine_aln and the ops are bit-identical to sp_affine_align_batch's (same encoding: a = allele = minimap2's query, b = consensus = its target).  Unlike that
 * call the map keeps no direction byte per cell: the forward pass leaves a checkpoint of the wave's state every 128 rows and the walk back re-runs one block of rows at a
 * time into LDS, so its scratch is bounded by the grid (pooled buffers of the context, no allocation on a warm context; sp_profile_get "pool:device" counts them).
 * A cell that found nothing (ok = 0) has no mapping (None in the reference): score 0, n_cigar 0, stats_mm2 -1.
 *   best_allele  the winner of sp_hla_score_consensus (the scan on the library's unit-cost alignments), unchanged
 *   best_mm2     score_read's running best (processed_match.rs:53-184) decided on the a = 5 alignments instead: the same scan run a second time on event rows and level
 *                records made from the ops.  A mapping with more than 255 edit bases (the event-row cap of the unit-cost scan) is no mapping to this scan: its level
 *                is absent there, as the level of an allele beyond the cap is absent in the unit-cost scan.  Its mapping is still handed out.  -1: nothing maps.
 *   stats_mm2    n_alleles * 6 in the order of `alleles`: cDNA (len, nm, unmapped), DNA (len, nm, unmapped) with len = the allele's length and unmapped = len - (a_end -
 *                a_start), as in sp_hla_best.mm2_stats; -1, -1, -1 = no mapping.
 * An alignment of more than 4,096 runs fails the call with SP_ERR_CAPACITY.  The handle owns everything its accessors point to, until sp_hla_map_free.  A call that
 * fails hands out no handle (*out = NULL): the reason is the context's sp_last_error; sp_hla_map_last_error is for the accessors (an index out of range). */
typedef struct sp_hla_map sp_hla_map;
int32_t sp_hla_map_consensus(sp_ctx* ctx, const sp_hla_db* db, uint32_t gene,
                             const char* cons_dna, uint32_t cons_dna_len, const char* cons_cdna, uint32_t cons_cdna_len,
                             int32_t require_dna, int32_t disable_cdna, sp_hla_map** out);
int32_t sp_hla_map_consensus_batch(sp_ctx* ctx, const sp_hla_db* db, uint32_t n, const uint32_t* genes,
                                   const char* const* cons_dna, const uint32_t* cons_dna_len, const char* const* cons_cdna, const uint32_t* cons_cdna_len,
                                   int32_t require_dna, int32_t disable_cdna, sp_hla_map** out);
/* the same from the hg38-forward consensus, as sp_hla_type_consensus takes it (placement, splice, gene strand): one item, or none when the consensus is empty or does
 * not align to its gene's reference */
int32_t sp_hla_map_type_consensus(sp_ctx* ctx, const sp_hla_db* db, uint32_t gene, const char* consensus_fwd, uint32_t consensus_len,
                                  int32_t require_dna, int32_t disable_cdna, sp_hla_map** out);
void sp_hla_map_free(sp_hla_map* map);
const char* sp_hla_map_last_error(const sp_hla_map* map);
uint32_t sp_hla_map_n_items(const sp_hla_map* map);
/* item `item` of the call: its gene, its allowed alleles in database order (n_alleles database indices), the two winners and stats_mm2; every output is optional */
int32_t sp_hla_map_item(const sp_hla_map* map, uint32_t item, uint32_t* gene, uint32_t* n_alleles, const uint32_t** alleles,
                        int32_t* best_allele, int32_t* best_mm2, const int32_t** stats_mm2);
/* the gene-strand consensus of a level (0 = cDNA, 1 = DNA): the target of the item's mappings at that level (not NUL-terminated; empty: cDNA scoring disabled) */
int32_t sp_hla_map_consensus_seq(const sp_hla_map* map, uint32_t item, int32_t level, const char** seq, uint32_t* len);
/* the mapping of allowed allele k of the item at a level: the alignment, the diagonal it was banded around (b_pos - a_pos), n_cigar ops at *cigar (NULL when 0) */
int32_t sp_hla_map_mapping(const sp_hla_map* map, uint32_t item, uint32_t k, int32_t level, sp_affine_aln* aln, int32_t* diag, uint32_t* n_cigar, const uint32_t** cigar);

/* ------------------------------------------------------------------ K2 ties: the alleles a call cannot tell from its winner
 * score_read keeps a strict running best (is_better_match, src/hla/processed_match.rs:103-184): the first allele in database order that nothing later beats is the
 * call, and every allele that ties with it is dropped without a word.  The _ex forms are the three map calls above plus `flags`; flags = 0 IS the call above (no
 * further launch, no further pooled memory, every output the same bytes).  SP_HLA_MAP_TIES adds one pass per scan (k2_ties_kernel: one workgroup per consensus, the
 * winner's records staged in LDS, no global atomic; pooled buffers, nothing allocated on a warm context): for the scan's winner W and every allowed allele X != W,
 * b_wx = better(W, X) and b_xw = better(X, W) on the level records, alignments and event rows the scan itself read, and whether the level loop of the rule (the overlap
 * edit counts, the presence rule; :113-168) or only the final mapping_score comparison (:174-183) decided.  The class of X is one byte:
 *   0 distinct       !b_xw, b_wx, decided in the level loop
 *   1 score_only     !b_xw, b_wx, decided by the mapping score alone: equal edits on every overlap, W wins the tie-break
 *   2 equal          !b_xw, !b_wx: indistinguishable; W is the call only because it comes first in database order
 *   3 beats_winner   b_xw: the relation is not transitive across different overlaps, so an allele beaten early in the scan can beat its final winner
 *   4 winner         X = W
 * A scan without a winner (-1) has class 0 for every allele and counts 0.
 * sp_hla_map_ties: scan 0 = the unit-cost scan (winner best_allele), 1 = the a = 5 scan (winner best_mm2); *cls = n_alleles class bytes in the order of `alleles`
 * (owned by the handle), counts[c] = the number of alleles of class c.  On a map made without SP_HLA_MAP_TIES: SP_ERR_INVALID_ARG, text in sp_hla_map_last_error. */
#define SP_HLA_MAP_TIES 1u
int32_t sp_hla_map_consensus_ex(sp_ctx* ctx, const sp_hla_db* db, uint32_t gene,
                                const char* cons_dna, uint32_t cons_dna_len, const char* cons_cdna, uint32_t cons_cdna_len,
                                int32_t require_dna, int32_t disable_cdna, uint32_t flags, sp_hla_map** out);
int32_t sp_hla_map_consensus_batch_ex(sp_ctx* ctx, const sp_hla_db* db, uint32_t n, const uint32_t* genes,
                                      const char* const* cons_dna, const uint32_t* cons_dna_len, const char* const* cons_cdna, const uint32_t* cons_cdna_len,
                                      int32_t require_dna, int32_t disable_cdna, uint32_t flags, sp_hla_map** out);
int32_t sp_hla_map_type_consensus_ex(sp_ctx* ctx, const sp_hla_db* db, uint32_t gene, const char* consensus_fwd, uint32_t consensus_len,
                                     int32_t require_dna, int32_t disable_cdna, uint32_t flags, sp_hla_map** out);
int32_t sp_hla_map_ties(const sp_hla_map* map, uint32_t item, int32_t scan /* 0 unit-cost, 1 mm2 */, const uint8_t** cls /* n_alleles, order of `alleles` */, uint32_t* counts /* 5 */);
/* `hla_ties.json` (host only; the layout of the other debug files: two-space indent).  One entry per gene; the file is keyed by gene in name order, then by
 * "consensus1" / "consensus2" (a consensus with present = 0 is left out, a gene with neither is omitted).  Each holds typed_allele (the call's; NULL: null), winner
 * (the scan's winner the classes are relative to; NULL: null -- the scan has none), scan ("unit_cost" | "mm2"), n_alleles, counts {distinct, score_only, equal,
 * beats_winner, winner} and three lists, "equal", "score_only" and "beats_winner", each {"names": [...], "more": n}: the names[k] of the alleles of that class in the
 * order given (database order), SP_HLA_TIES_MAX_NAMES at the most; "more": the number left out, only when there are any.  out / cap / needed as sp_cyp_alleles_json. */
#define SP_HLA_TIES_MAX_NAMES 256u
typedef struct {
    const char* gene;
    int32_t present[2];                 /* the consensus has a row */
    int32_t scan[2];                    /* 0 unit-cost, 1 mm2 */
    const char* typed_allele[2];        /* the star string of the call for each consensus */
    const char* winner[2];              /* the star string of the scan's winner */
    uint32_t n_alleles[2];
    const uint8_t* cls[2];              /* n_alleles class bytes (sp_hla_map_ties) */
    const uint32_t* counts[2];          /* 5 (sp_hla_map_ties) */
    const char* const* names[2];        /* n_alleles full star names ("HLA-A*01:01:01:01") in the order of cls */
} sp_hla_ties_entry;
int32_t sp_hla_ties_json(const sp_hla_ties_entry* entries, uint32_t n_entries, char* out, uint64_t cap, uint64_t* needed);

/* ------------------------------------------------------------------ K5: CYP2D6 chain-pair likelihood search
 * Replaces find_best_chain_pair (src/cyp2d6/chaining.rs:223-592) with containment_score (:683-731),
 * get_multinomial_score (:854-903), count_unexpected_alleles (:794-819), unexpected_count (:739-775),
 * count_inferred_edges (:828-840), check_chain_inferrences (:603-674) and multinomial_ln_pmf (src/util/stats.rs:11-37).
 * The grammar / enumeration runs on the host exactly as in the reference (LIFO DFS, copy number <= 3); every unordered
 * chain pair is then scored by one GPU thread in f64 with the reference's operation order, and the winner is
 * min (primary_score, i, j) -- what the reference's top-10 heap returns (chaining.rs:188-196,565-573).
 *   hap_type       Cyp2d6RegionType per consensus region (src/cyp2d6/region_label.rs:7-24), SP_CYP_* below
 *   hap_subtype    subtype label or NULL
 *   translate / connections / singletons   the three Cyp2d6Config tables (src/cyp2d6/definitions.rs:242-301)
 *   reads          in BTreeMap (qname) order: read r owns chains [read_chain_off[r], read_chain_off[r+1]) (obs_chains) and
 *                  weight rows [read_w_off[r], read_w_off[r+1]) (chain_scores); a row holds n_haps (edit distance, overlap) pairs
 * Returns SP_OK, or SP_ERR_NO_CHAINING_HEAD / SP_ERR_NO_CHAINS_FOUND / SP_ERR_NO_SCORE_PAIRS (CallerError, expected failures).
 */
enum { SP_CYP_UNKNOWN = 0, SP_CYP_REP6 = 1, SP_CYP_CYP2D6 = 2, SP_CYP_LINK_REGION = 3, SP_CYP_REP7 = 4, SP_CYP_SPACER = 5,
       SP_CYP_CYP2D7 = 6, SP_CYP_DELETION = 7, SP_CYP_HYBRID = 8, SP_CYP_FALSE_ALLELE = 9 };
#define SP_MAX_CHAIN 64

typedef struct {
    uint32_t n_haps;
    const int32_t* hap_type;
    const char* const* hap_subtype;
    uint32_t n_translate; const char* const* translate_key; const char* const* translate_val;
    uint32_t n_connections; const char* const* connection_a; const char* const* connection_b;
    uint32_t n_singletons; const char* const* singletons;
    uint32_t n_reads;
    const uint32_t* read_chain_off;     /* n_reads+1 */
    const uint32_t* chain_off;          /* n_chains+1 */
    const uint32_t* chain_items;
    const uint32_t* read_w_off;         /* n_reads+1 */
    const uint64_t* w_ed;               /* [row][n_haps] */
    const double*   w_ov;               /* [row][n_haps] */
    int32_t infer_connections, normalize_all_alleles, ignore_chain_label_limits;
    double lasso_penalty, ln_ed_penalty, unexpected_chain_penalty, inferred_edge_penalty;   /* ChainPenalties, chaining.rs:107-139 */
} sp_chain_problem;

typedef struct {
    int32_t n_possible;                 /* enumerated chains */
    int32_t index1, index2;             /* winning pair (i <= j) in enumeration order */
    int32_t n1, n2;
    int32_t chain1[SP_MAX_CHAIN], chain2[SP_MAX_CHAIN];    /* the pair, sorted (chaining.rs:568-573) */
    double score, ln_ed_penalty, mn_llh_penalty, allele_expected_penalty, unexpected_chain_penalty, inferred_chain_penalty;
    uint64_t edit_distance;
    uint64_t n_pairs_scored;            /* pairs whose read-level terms were evaluated on the GPU */
} sp_chain_result;

int32_t sp_cyp_best_chain_pair(sp_ctx* ctx, const sp_chain_problem* problem, sp_chain_result* result);

/* The runner-up pairs: the content of the reference's 10-entry heap (chaining.rs:404-405,515-526), which it prints at debug level (:540-557).
 * Among the pairs i <= j whose get_multinomial_score is valid, the max_alts (1..64) smallest under (primary_score, i, j), ascending -- ChainScore's Ord
 * (:188-196) with i, j in enumeration order; entry 0 is sp_cyp_best_chain_pair's winner, field for field.  The list does not depend on the launch order or on
 * the kernel that ran: a pair is skipped only when its partial cost is strictly above a proven upper bound of the max_alts-th best complete score.
 *   alts          max_alts records; *n_alts = min(max_alts, valid pairs) are written
 *   hap_counts    optional [max_alts][n_haps]: copies of each region in the pair
 *   hap_weights   optional [max_alts][n_haps]: the coverage the reads gave each region (the f64 sums the score was made from)
 *   best          optional: entry 0 in the old record, with n_possible and n_pairs_scored
 * Statuses as sp_cyp_best_chain_pair.  sp_cyp_possible_chains (host only; ctx may be NULL: it only receives the error text) lists the chains index1 / index2 refer to, in enumeration order:
 * chain c is items[chain_off[c] .. chain_off[c+1]); *n_chains / *n_items are always set, SP_ERR_CAPACITY when off_cap < n_chains + 1 or items_cap < n_items. */
#define SP_CYP_ALTERNATIVES 10         /* the reference's heap size: what the whole-sample switch asks for */
typedef struct {
    int32_t index1, index2;             /* i <= j, enumeration order */
    int32_t n1, n2;
    int32_t chain1[SP_MAX_CHAIN], chain2[SP_MAX_CHAIN];    /* sorted as in sp_chain_result */
    double score, ln_ed_penalty, mn_llh_penalty, allele_expected_penalty, unexpected_chain_penalty, inferred_chain_penalty;
    uint64_t edit_distance;
    uint32_t unmet_observations;        /* reads none of whose putative chains is a sub-chain of either chain (chaining.rs:427-440) */
    uint32_t reserved_;
} sp_chain_alt;

int32_t sp_cyp_best_chain_pairs(sp_ctx* ctx, const sp_chain_problem* problem, uint32_t max_alts, sp_chain_alt* alts, uint32_t* n_alts,
                                int32_t* hap_counts, double* hap_weights, sp_chain_result* best);
int32_t sp_cyp_possible_chains(sp_ctx* ctx, const sp_chain_problem* problem, uint32_t* chain_off, uint32_t off_cap, uint32_t* items, uint32_t items_cap,
                               uint32_t* n_chains, uint32_t* n_items);
/* `cyp2d6_alternatives.json` (sp_starphase_set_cyp_alternatives), host only: {"n_possible_chains", "n_pairs_scored"?, "alternatives": [...]}, best first; an
 * alternative has rank (1: the call), diplotype (convert_chain_to_hap of the two chains, sub-allele detail, "hap1/hap2"), chains (two lists of "<index>_<label>" region names, the
 * naming of DanglingAllele, chaining.rs:587), score, delta_to_best, the five components, edit_distance, unmet_observations and coverage
 * ([{"region", "copies", "observed"}] for the regions with copies > 0; [] without hap_counts).  n_pairs_scored is written only when the pointer is given (the
 * whole-sample call leaves it out: it differs from run to run).  problem: the labels and the translation table.  out / cap / needed as sp_cyp_alleles_json. */
int32_t sp_cyp_alternatives_json(const sp_chain_problem* problem, uint32_t n_possible_chains, const uint64_t* n_pairs_scored, const sp_chain_alt* alts, uint32_t n_alts,
                                 const int32_t* hap_counts, const double* hap_weights, char* out, uint64_t cap, uint64_t* needed);

/* A pair read by read: the per-read quantities every read-dependent term of a pair's score is made from -- containment_score (chaining.rs:683-731) and the is_sub
 * loop (:427-440) -- which the search reduces away and the reference never hands out.  For any n_pairs (1..64) pairs (index1[k] <= index2[k], enumeration order:
 * sp_cyp_possible_chains), whether or not get_multinomial_score finds them valid and whatever the search ranks.  reads[k * n_reads + r], for pair (i, j) = (index1[k],
 * index2[k]) and read r with wl weight rows:
 *   optimum = the sum over the rows of the smallest edit distance of the row, worst = the sum of the largest
 *   the chains are taken in the order i, then j (i == j: the same chain twice, as the reference does: mask2 == mask1); a chain shorter than wl has no start; the
 *   starts s = 0 .. len - wl ascend; best begins at 2 * worst, a strictly smaller window total clears the placements, an equal one adds to them
 *   mask1 / mask2  bit s: start s of chain i / chain j reaches best (SP_MAX_CHAIN is 64: a word holds every start)
 *   n_best         popcount(mask1) + popcount(mask2): the divisor of split_frac; 0 when the read is longer than both chains
 *   excess_ed      best - optimum (no placement: 2 * worst - optimum): what the reference adds to read_combined_ed
 *   supported      1 when an observed chain of the read is a run of consecutive regions of chain i or of chain j; a read without observed chains is not
 * A read with observed chains but no weight rows (wl = 0) is treated as the search treats it: every start 0 .. len of both chains is a best placement of total 0
 * (the masks hold the starts below 64), excess_ed 0; it adds nothing to any coverage sum.
 * edit_distance[k] (the saturating sum of excess_ed) and unmet_observations[k] (the reads with supported == 0) are the column sums, made on the device; both optional,
 * only what is asked for is downloaded (each total by itself).  They equal sp_chain_alt's fields for a pair sp_cyp_best_chain_pairs lists, and hap_weights[k] is the sum over the reads in
 * order, chain i's starts ascending, then chain j's, rows ascending, of (1 / n_best) * w_ov[row][region].
 * Statuses as sp_cyp_best_chain_pair for the enumeration (SP_ERR_NO_SCORE_PAIRS does not occur: nothing is ranked); SP_ERR_INVALID_ARG for n_pairs outside 1..64, an
 * index outside [0, n_possible) or index1 > index2.  Pooled memory only. */
typedef struct {
    uint64_t mask1, mask2;
    uint64_t excess_ed;
    uint32_t n_best;
    uint8_t supported;
    uint8_t reserved_[3];
} sp_chain_pair_read;
int32_t sp_cyp_chain_pair_reads(sp_ctx* ctx, const sp_chain_problem* problem, uint32_t n_pairs, const int32_t* index1, const int32_t* index2,
                                sp_chain_pair_read* reads, uint64_t* edit_distance, uint32_t* unmet_observations);
/* The observed-chain table (host only; ctx may be NULL): chain_frequency (caller.rs:544-550) -- the distinct observed chains in lexicographic order
 * (BTreeMap<Vec<usize>>), chain c = items[chain_off[c] .. chain_off[c+1]) with frequency[c] = the sum over the reads in problem order of 1 / (chains of the read) per
 * occurrence -- and what generate_debug_graph derives from it (visualization.rs:32-45): single_counts[n_haps] (optional) and the edges (edge_from, edge_to) in
 * lexicographic order with edge_weight, both summed over the chains in table order.  The numbers of the reference's cyp2d6_link_graph.svg.  frequency has room for
 * off_cap entries.  *n_chains / *n_items / *n_edges and single_counts are always set; SP_ERR_CAPACITY when off_cap < n_chains + 1, items_cap < n_items or
 * edge_cap < n_edges. */
int32_t sp_cyp_observed_chains(sp_ctx* ctx, const sp_chain_problem* problem, uint32_t* chain_off, uint32_t off_cap, uint32_t* items, uint32_t items_cap, double* frequency,
                               double* single_counts, uint32_t* edge_from, uint32_t* edge_to, double* edge_weight, uint32_t edge_cap,
                               uint32_t* n_chains, uint32_t* n_items, uint32_t* n_edges);
/* `cyp2d6_alternative_reads.json` (sp_starphase_set_cyp_alternative_reads), host only: {"observed": {...}, "alternatives": [...]}.
 * observed: chains [{"chain": ["<index>_<label>", ...], "reads"}], regions [{"region", "reads"}] (the regions with a non-zero total; [] without single_counts) and
 * links [{"from", "to", "reads"}] -- the table of sp_cyp_observed_chains, region names as in cyp2d6_alternatives.json.
 * alternatives: one object per alts[k], in the order given, with reads[k * n_reads + r] its records: rank, diplotype and chains (as sp_cyp_alternatives_json spells
 * them: the pair sorted), hap1_chain (1 or 2: which entry of chains is the chain index1 names -- hap1 of the placements; hap2 is the other, or the same chain when
 * index1 == index2), edit_distance, unmet_observations (the record's), for rank > 1 reads_decided_for / reads_decided_against (the reads whose excess_ed is larger /
 * smaller than under rank 1) and reads: the reads that are not neutral -- neutral: excess_ed == 0, supported, and the same excess_ed as under rank 1 -- as {"read",
 * "excess_ed", "delta_to_best" (signed: against rank 1), "supported", "placements": ["hap1@<start>", ..., "hap2@<start>", ...]}.  read_names: n_reads names, or NULL
 * (or a NULL entry) for "read <r>".  index1 / index2 must name chains of the problem.  out / cap / needed as sp_cyp_alleles_json. */
int32_t sp_cyp_alternative_reads_json(const sp_chain_problem* problem, const sp_chain_alt* alts, uint32_t n_alts, const sp_chain_pair_read* reads, const char* const* read_names,
                                      const uint32_t* obs_chain_off, const uint32_t* obs_items, const double* obs_frequency, uint32_t n_obs_chains,
                                      const double* single_counts, const uint32_t* edge_from, const uint32_t* edge_to, const double* edge_weight, uint32_t n_edges,
                                      char* out, uint64_t cap, uint64_t* needed);

/* ------------------------------------------------------------------ K3: CYP2D6 template search in reads
 * Replaces Cyp2d6Extractor::find_base_type_in_sequence (src/cyp2d6/haplotyper.rs:142-315) for a batch of reads:
 * every template (D6, D7, *5 signature, hybrids, REP6/REP7, spacer, link_region -- given in the reference's key order,
 * i.e. sorted by full_allele(), :175-183) is placed on every read (up to 4 placements), hits with more than 5 % edits
 * are dropped (un-mapped template bases count only for *5 / REP6 / REP7, :185-191,228-232), hits are sorted by
 * (start, end), overlapping hits (> 0.9 of the shorter) collapse to the better one with *5 priority (:260-296), and hits
 * whose penalised fraction exceeds max_missing_frac are dropped (:303-306).
 * hits: grouped by read, in output order; returns the total in n_hits (may exceed hits_cap: call again with more room). */
typedef struct {
    int32_t read, template_idx;
    int32_t start, end;                 /* region on the read */
    int32_t seq_len, nm, unmapped;      /* MappingStats of the template */
    int32_t clip_start, clip_end;
    /* the hit re-scored the reference's way (two-piece affine gaps, end clipping; 256 diagonals: sp_affine_rescore_batch): minimap2's NM, region on the read and
     * template span for this mapping; mm2_score 0 = not re-scored (context option "mm2_rescore" 0).  The filters above use the library's own counts. */
    int32_t mm2_score, mm2_nm;
    int32_t mm2_start, mm2_end;         /* region on the read */
    int32_t mm2_q_start, mm2_q_end;     /* span on the template: unmapped = seq_len - (mm2_q_end - mm2_q_start), clips = mm2_q_start, seq_len - mm2_q_end */
} sp_region_hit;

int32_t sp_cyp_find_regions(sp_ctx* ctx, const sp_seqset* templates, const int32_t* template_type, const sp_seqset* reads,
                            double max_missing_frac, sp_region_hit* hits, uint64_t hits_cap, uint64_t* n_hits);

/* ------------------------------------------------------------------ K4: consensus weights of read segments
 * Replaces weight_sequence (src/cyp2d6/chaining.rs:28-103) for a batch of read segments: every allowed consensus
 * (allowed[c] = label.is_allowed_label()) is placed on every segment; ed[s][c] = nm + un-mapped segment bases,
 * ov[s][c] = 1 - clipped consensus fraction, defaults (segment length, 0.0); kept[s] = 0 when the reference returns the
 * empty vector (best penalised fraction > 0.05).  With the context option "mm2_rescore" (default 1) a placement whose nm + un-mapped bases are within 16 of the
 * segment's smallest over the allowed consensuses enters with the reference's numbers -- re-scored with minimap2's two-piece affine scores on 256 diagonals
 * (sp_affine_rescore_batch): its NM, spans and clips --, the others with the unit-cost count (a lower bound of the other). */
int32_t sp_cyp_weight_segments(sp_ctx* ctx, const sp_seqset* consensus, const uint8_t* allowed, const sp_seqset* segments,
                               uint64_t* ed, double* ov, uint8_t* kept);

/* ------------------------------------------------------------------ K7: star-allele vector scoring
 * Replaces the scoring loop of Cyp2d6Extractor::assign_haplotype (src/cyp2d6/haplotyper.rs:470-524): for each typed
 * sequence, its per-variant state vector (0 ref, 1 alt, 2 ambiguous, 3 unset) is compared with the 0/1 definition of
 * every star allele; score = (matches at VI variants, matches at all variants), 2 always matches, 3 never does.
 *   hap_matrix   n_alleles x n_variants (0/1), alleles in haplotype_lookup (BTreeMap) order
 *   is_vi        n_variants (LoadedVariants::is_vi)
 *   states       n_seqs x n_variants
 * Outputs per sequence: best (vi_match, all_match) (starting from the (0,0) of the Unknown label, :472-474) and, in
 * tie_mask (n_seqs x n_alleles bytes), which alleles reach it; no allele beats or ties (0,0) => all zero.
 * The caller resolves ties by sorting full_allele() strings (:531-547). */
int32_t sp_cyp_score_alleles(sp_ctx* ctx, uint32_t n_variants, uint32_t n_alleles, const uint8_t* hap_matrix, const uint8_t* is_vi,
                             uint32_t n_seqs, const uint8_t* states, uint32_t* best_vi, uint32_t* best_all, uint8_t* tie_mask);

/* ------------------------------------------------------------------ K9: per-variant state of typed sequences
 * The role of WFAGraph::from_reference_variants + edit_distance_with_pruning + the traversed-node loop of assign_haplotype
 * (src/cyp2d6/haplotyper.rs:371-468): which allele of every database variant a consensus carries.  hiphase v1.2.1 is not on disk;
 * the contract: the sequence is placed on the backbone (GPU alignment with traceback); for every variant whose
 * reference span lies inside the aligned part, the sequence window facing [p - 24, p + |ref| + 24) is compared (global edit
 * distance, one GPU thread per pair) with that backbone window carrying the reference allele and carrying the alternate allele:
 * 0 = closer to the reference, 1 = closer to the alternate, 2 = equally close (ambiguous), 3 = not covered / not aligned.
 *   backbone    the CYP2D6_wfa_backbone slice of the reference; var_pos 0-based on it; var_ref / var_alt normalised ACGT alleles
 *   states      sp_seqset_count(seqs) * n_variants, ready for sp_cyp_score_alleles;  alns (optional) placement of every sequence */
int32_t sp_cyp_variant_states(sp_ctx* ctx, const sp_seqset* seqs, const char* backbone, uint32_t backbone_len, uint32_t n_variants,
                              const int32_t* var_pos, const char* const* var_ref, const char* const* var_alt,
                              uint8_t* states, sp_aln* alns);

/* ------------------------------------------------------------------ CYP2D6, reads to diplotype
 * diplotype_cyp2d6 (src/cyp2d6/caller.rs:39-741) on top of K3 / K8 / K9 / K7 / K4 / K5, without I/O and debug artefacts:
 * regions of interest (:126-139) -> consensus inputs with offsets and seeds (:176-245) -> multi-way consensus (:268) ->
 * merge_consensus_results (:750-898) -> typing of every consensus with find_full_type_in_sequence / assign_haplotype
 * (src/cyp2d6/haplotyper.rs:326-602) and duplicate detection (:331-375) -> weights, chains, best chain pair (:429-640) ->
 * haplotype strings (:660-690).
 *   templates          Cyp2d6Extractor::hybrid_sequences in full_allele() order (haplotyper.rs:175-183) with type, subtype label and
 *                      template_deep[t] = 1 when the label is in mapped_hybrids (typed further by its variants)
 *   backbone, var_*    the CYP2D6_wfa_backbone slice and LoadedVariants::ordered_variants on it (0-based), is_vi flags
 *   allele_subtype / hap_matrix   haplotype_lookup in BTreeMap order: star-allele label ("4.001") and its 0/1 vector
 *   translate / connections / singletons   the three Cyp2d6Config tables
 * call->status: 0 called, 1 = no reads (NO_READS), 7 = chain collapse, 16/17/18 = CallerError (NO_MATCH).  hap1/hap2 carry the
 * sub-allele strings, core1/core2 the core-allele strings (Cyp2d6DetailLevel::SubAlleles / CoreAlleles). */
typedef struct {
    const sp_seqset* templates; const int32_t* template_type; const char* const* template_subtype; const uint8_t* template_deep;
    const char* backbone; uint32_t backbone_len;
    uint32_t n_variants; const int32_t* var_pos; const char* const* var_ref; const char* const* var_alt; const uint8_t* var_is_vi;
    uint32_t n_alleles; const char* const* allele_subtype; const uint8_t* hap_matrix;
    uint32_t n_translate; const char* const* translate_key; const char* const* translate_val;
    uint32_t n_connections; const char* const* connection_a; const char* const* connection_b;
    uint32_t n_singletons; const char* const* singletons;
    int32_t min_consensus_count, dual_max_ed_delta; double min_consensus_fraction;
    int32_t infer_connections, normalize_d6_only;
    const char* const* var_label;                 /* LoadedVariants::variant_label per variant, for the deep strings of the call; NULL: none are listed */
} sp_cyp_problem;

#define SP_CYP_MAXCONS 64
typedef struct {
    int32_t status;
    int32_t n_consensus;                          /* final consensus regions (hap_regions) */
    int32_t cons_type[SP_CYP_MAXCONS];            /* SP_CYP_* after typing, duplicate and false-allele marking */
    char    cons_subtype[SP_CYP_MAXCONS][48];     /* "" = none */
    int32_t n1, n2; int32_t chain1[SP_MAX_CHAIN], chain2[SP_MAX_CHAIN];
    double  score;
    char hap1[256], hap2[256], core1[256], core2[256];
    /* Cyp2d6DetailLevel::DeepAlleles (src/cyp2d6/caller.rs:907-957, Cyp2d6Region::deep_label, src/cyp2d6/region.rs:47-91): every reported
     * region as "(<index>_<full allele>[ +label | -label | ?label ...])" with the variants that differ from the assigned star allele --
     * the haplotypes of the InexactDiplotype the reference stores for CYP2D6 (:711-716,737); truncated to the buffer */
    char deep1[2048], deep2[2048];
    int32_t searches_gave_up;                     /* two-way searches of the multi-way consensus that ended without a complete node: their groups stayed whole */
    int32_t reserved_;
} sp_cyp_call;

int32_t sp_cyp_diplotype(sp_ctx* ctx, const sp_cyp_problem* problem, const sp_seqset* reads, sp_cyp_call* call,
                         char* consensus /* optional: SP_CYP_MAXCONS * cons_cap bytes */, uint32_t cons_cap);

/* One GPU's share of a cohort: the call of sp_cyp_diplotype for each of n_samples read sets against the same problem.  The samples are
 * spread over the context's streams (sp_ctx_set_option), one host thread per stream for the length of the call; calls[i], the
 * consensus block of sample i (optional: n_samples * SP_CYP_MAXCONS * cons_cap bytes) and sample_rc[i] (optional) are what the single
 * call would give.  Returns the first status that is not SP_OK. */
int32_t sp_cyp_diplotype_cohort(sp_ctx* ctx, const sp_cyp_problem* problem, uint32_t n_samples, const sp_seqset* const* reads, sp_cyp_call* calls,
                                char* consensus, uint32_t cons_cap, int32_t* sample_rc);

/* The same call, also handing out Cyp2d6Region::variants of every final consensus region (assign_haplotype,
 * src/cyp2d6/haplotyper.rs:546-595): has_variants[h] = 1 when region h carries a list (typed as a CYP2D6 star allele), and
 * state[h * n_variants + v] is the VariantAlleleRelationship of variant v against the assigned allele in the codes of
 * sp_inexact_haplotype (1 Match .. 7 UnknownMissing), 255 = not listed (reference where the allele has the reference).
 * state: caller's buffer of SP_CYP_MAXCONS * n_variants bytes (NULL: only has_variants is filled).
 * sp_cyp_alleles_json writes the `cyp2d6_alleles.json` debug file (DeeplotypeDebug, src/cyp2d6/debug.rs:10-70; caller.rs:703-707) from
 * the call and these lists: the two haplotypes in deep / sub-allele / core form and {index_label: [RegionVariant]} in key order.
 * out / cap: the text is copied NUL-terminated; *needed = bytes needed incl. the NUL; SP_ERR_CAPACITY when it did not fit. */
typedef struct { uint8_t has_variants[SP_CYP_MAXCONS]; uint8_t* state; } sp_cyp_region_variants;
int32_t sp_cyp_diplotype_detailed(sp_ctx* ctx, const sp_cyp_problem* problem, const sp_seqset* reads, sp_cyp_call* call,
                                  char* consensus, uint32_t cons_cap, sp_cyp_region_variants* region_variants /* optional */);
int32_t sp_cyp_alleles_json(const sp_cyp_problem* problem, const sp_cyp_call* call, const sp_cyp_region_variants* region_variants,
                            char* out, uint64_t cap, uint64_t* needed);
/* The same call, also handing out the read assignments behind PgxGeneDetails::multi_mapping_details (src/cyp2d6/caller.rs:434-565): for every read
 * (in the order of `reads` = QNAME order) whose chain set is exactly one chain after the chains with a consensus nothing maps to uniquely were
 * removed, one record per element of that chain, paired in order with the read's regions of interest (Rust's zip: the shorter list ends it) --
 * the region's read range [read_start, read_end), the consensus index and its index_label ("<index>_<full allele>", the label before
 * mark_false_allele, as the reference reads it).  mappings: cap records; *n_mappings = the number there are (SP_ERR_CAPACITY when more than
 * cap: the call itself is complete, call again with more room for the list).  No records when call->status is not 0. */
typedef struct { uint32_t read, consensus; uint64_t read_start, read_end; char index_label[64]; } sp_cyp_read_mapping;
int32_t sp_cyp_diplotype_mappings(sp_ctx* ctx, const sp_cyp_problem* problem, const sp_seqset* reads, sp_cyp_call* call, char* consensus, uint32_t cons_cap,
                                  sp_cyp_region_variants* region_variants /* optional */, sp_cyp_read_mapping* mappings, uint64_t cap, uint64_t* n_mappings);
/* sp_cyp_diplotype_cohort that also hands out, per sample, what sp_cyp_diplotype_mappings gives for it: region_variants[i] (optional; n_samples
 * entries, each with its own state block) and the read mappings of sample i at mappings[mapping_off[i] .. mapping_off[i + 1]) (mapping_off: n_samples + 1
 * entries, always filled; SP_ERR_CAPACITY when mapping_off[n_samples] > cap: the calls are complete, call again with more room for the list). */
int32_t sp_cyp_diplotype_cohort_mappings(sp_ctx* ctx, const sp_cyp_problem* problem, uint32_t n_samples, const sp_seqset* const* reads, sp_cyp_call* calls,
                                         char* consensus, uint32_t cons_cap, sp_cyp_region_variants* region_variants /* optional */,
                                         sp_cyp_read_mapping* mappings, uint64_t cap, uint64_t* mapping_off, int32_t* sample_rc);

/* ------------------------------------------------------------------ CYP2D6 consensus support: how well the member reads back each consensus region of a call
 * The table of sp_hla_consensus_support (below) for the consensus regions of a CYP2D6 call; an output of this library's own.  call / consensus / cons_cap / mappings as
 * sp_cyp_diplotype_mappings returned them for `reads`.
 *   members    of consensus h: the mapping records with .consensus == h -- the reads with exactly one chain, the reference's rule for multi_mapping_details, kept as it
 *              is: a read with several chains backs no consensus here.  A read with several regions on one consensus is several members.
 *   pairs      query = reads[r][read_start, read_end), target = consensus h as the call returned it.  Orientation: the regions of interest are cut out of the reads as
 *              uploaded (sp_region_hit has no strand, the segments are forward views of the reads) and every consensus is built from such segments, so reads and
 *              consensuses share one orientation; there is no strand handling.
 *   alignment  sp_anchor_batch(A = the consensuses, B = the segments) gives the diagonal (negated, as in the HLA pass); sp_align_pileup_batch at the map-hifi scores
 *              {1, 4, 6, 2, 26, 1, 1} on 64 diagonals.  There is NO second try on 256 diagonals (the HLA pass has one): a member without an anchor (0 votes) or
 *              without an alignment on 64 diagonals is counted in n_unaligned and left out; it is not an error.
 * col_offset (n_consensus + 1 entries, always filled): consensus h owns cols[col_offset[h] .. col_offset[h + 1]); cols may be NULL (cols_cap ignored: no table is
 * downloaded, the summaries are computed on the device all the same); SP_ERR_CAPACITY when cols is given and col_offset[n_consensus] > cols_cap (call again with more
 * room).  summaries: n_consensus records.  call->status != 0: SP_OK, col_offset all 0, the summaries zeroed, nothing launched.
 * sp_cyp_consensus_support_cohort: n_samples calls in one pass -- one segment set, one anchor launch, one sp_align_pileup_batch.  calls[i], the consensus block of sample i
 * (n_samples * SP_CYP_MAXCONS * cons_cap bytes) and mappings[mapping_off[i] .. mapping_off[i + 1]) as sp_cyp_diplotype_cohort_mappings returned them; col_offset:
 * n_samples * SP_CYP_MAXCONS + 1 entries, summaries: n_samples * SP_CYP_MAXCONS (consensus h of sample i at i * SP_CYP_MAXCONS + h; the slots behind n_consensus own no
 * columns and are zeroed).
 * sp_cyp_support_json: `cyp2d6_consensus_support.json` (host only; two-space indent, the layout of consensus_support.json): one entry per consensus region in consensus
 * order, keyed by its index_label ("<index>_<full allele>", the key of cyp2d6_alleles.json), each with n_members, n_aligned, n_unaligned, length, min_depth,
 * median_depth, n_contested, region_type (the full allele label of cons_type / cons_subtype) and contested = [{pos, depth, eq, x: [a, c, g, t], del, ins,
 * consensus_base}].  col_offset / cols / summaries: n_consensus (+ 1) entries as sp_cyp_consensus_support filled them (cols must be given).  A call with
 * status != 0 has no entries: the text is {} (the whole-sample call writes no file for it).  out / cap / needed as sp_cyp_alleles_json. */
int32_t sp_cyp_consensus_support(sp_ctx* ctx, const sp_seqset* reads, const sp_cyp_call* call, const char* consensus, uint32_t cons_cap,
                                 const sp_cyp_read_mapping* mappings, uint64_t n_mappings, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap,
                                 sp_support_summary* summaries);
int32_t sp_cyp_consensus_support_cohort(sp_ctx* ctx, uint32_t n_samples, const sp_seqset* const* reads, const sp_cyp_call* calls, const char* consensus, uint32_t cons_cap,
                                        const sp_cyp_read_mapping* mappings, const uint64_t* mapping_off, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap,
                                        sp_support_summary* summaries);
int32_t sp_cyp_support_json(const sp_cyp_call* call, const char* consensus, uint32_t cons_cap, const uint64_t* col_offset, const sp_pileup_col* cols,
                            const sp_support_summary* summaries, char* out, uint64_t cap, uint64_t* needed);
/* The same calls with the insertion list of sp_align_pileup_ins_batch (ins / ins_cap / n_ins as there; ins == NULL is the call above: nothing else is launched).  Same
 * members, band and rule.  col is in the call's col_offset space; first_pair is the index of the member's record in `mappings`, first_qpos the run's position in the
 * member's segment (read position - read_start).  sp_cyp_support_json_ins: every contested entry with 2 * ins > depth gains "insertions" (and "other", "more") as
 * sp_consensus_support_json_ins writes them; read_names (optional): the QNAME of read r of the sample at read_names[r], n_read_names entries; ins == NULL or
 * n_ins == 0: the bytes of sp_cyp_support_json. */
int32_t sp_cyp_consensus_support_ins(sp_ctx* ctx, const sp_seqset* reads, const sp_cyp_call* call, const char* consensus, uint32_t cons_cap,
                                     const sp_cyp_read_mapping* mappings, uint64_t n_mappings, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap,
                                     sp_support_summary* summaries, sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins);
int32_t sp_cyp_consensus_support_cohort_ins(sp_ctx* ctx, uint32_t n_samples, const sp_seqset* const* reads, const sp_cyp_call* calls, const char* consensus, uint32_t cons_cap,
                                            const sp_cyp_read_mapping* mappings, const uint64_t* mapping_off, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap,
                                            sp_support_summary* summaries, sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins);
int32_t sp_cyp_support_json_ins(const sp_cyp_call* call, const char* consensus, uint32_t cons_cap, const uint64_t* col_offset, const sp_pileup_col* cols,
                                const sp_support_summary* summaries, const sp_pileup_ins* ins, uint64_t n_ins, const sp_cyp_read_mapping* mappings, uint64_t n_mappings,
                                const char* const* read_names, uint32_t n_read_names, char* out, uint64_t cap, uint64_t* needed);
/* The _ins forms with the haplotype list of sp_align_pileup_hap_batch as well (haps / hap_cap / n_haps / heads as there; haps == NULL is the _ins form: nothing else is
 * launched).  target is the consensus' slot of col_offset (h for the single call, sample * SP_CYP_MAXCONS + h for the cohort); heads: one per slot (n_consensus for the
 * single call, n_samples * SP_CYP_MAXCONS for the cohort), an unused slot's is empty; first_pair is the index of the member's record in `mappings`.  Either list may be
 * asked for without the other; SP_ERR_CAPACITY names the list that did not fit by its count (n_ins > ins_cap, n_haps > hap_cap), the other one is complete.
 * sp_cyp_support_json_hap: sp_cyp_support_json_ins with a list: consensus h is target target0 + h of it, its head heads[target0 + h] (target0 = 0 for the list of the
 * single call, sample * SP_CYP_MAXCONS for a sample of the cohort call): a region whose head has n_cols > 0 and records gains
 * "haplotypes" as sp_consensus_support_json_hap writes it, behind "contested"; haps == NULL or n_haps == 0: the bytes of sp_cyp_support_json_ins. */
int32_t sp_cyp_consensus_support_hap(sp_ctx* ctx, const sp_seqset* reads, const sp_cyp_call* call, const char* consensus, uint32_t cons_cap,
                                     const sp_cyp_read_mapping* mappings, uint64_t n_mappings, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap,
                                     sp_support_summary* summaries, sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins,
                                     sp_support_hap* haps, uint64_t hap_cap, uint64_t* n_haps, sp_support_hap_head* heads);
int32_t sp_cyp_consensus_support_cohort_hap(sp_ctx* ctx, uint32_t n_samples, const sp_seqset* const* reads, const sp_cyp_call* calls, const char* consensus, uint32_t cons_cap,
                                            const sp_cyp_read_mapping* mappings, const uint64_t* mapping_off, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap,
                                            sp_support_summary* summaries, sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins,
                                            sp_support_hap* haps, uint64_t hap_cap, uint64_t* n_haps, sp_support_hap_head* heads);
int32_t sp_cyp_support_json_hap(const sp_cyp_call* call, const char* consensus, uint32_t cons_cap, const uint64_t* col_offset, const sp_pileup_col* cols,
                                const sp_support_summary* summaries, const sp_pileup_ins* ins, uint64_t n_ins, const sp_support_hap* haps, uint64_t n_haps,
                                const sp_support_hap_head* heads, uint64_t target0, const sp_cyp_read_mapping* mappings, uint64_t n_mappings,
                                const char* const* read_names, uint32_t n_read_names, char* out, uint64_t cap, uint64_t* needed);

/* ------------------------------------------------------------------ cyp2d6_alleles.vcf.gz: the variants of the typed regions as a VCF, with read support
 * write_cyp2d6_vcf (src/cyp2d6/vcf_writer.rs; caller.rs:410-413): one haploid sample column per region typed as a CYP2D6 star allele (has_variants[h] == 1), in
 * region order, named by its index label "<index>_<full allele>" (the key of cyp2d6_alleles.json), and one record per database variant that at least one such region
 * lists (state != 255), in variant-table order.  GT: AmbiguousUnexpected, AmbiguousMissing -> '.'; Match, Unexpected -> 1; everything else, and a region that does not
 * list the variant -> 0.  The reference leaves QUAL and depth open; this library fills in two FORMAT fields of its own from window support (above):
 *   SR  member reads of the region's consensus whose alignment spans the variant's window on that consensus      CR  those of them that match the consensus at every base of it
 * They say how well the reads agree with the CONSENSUS around the variant -- not REF / ALT read counts: a region whose consensus carries ALT has CR reads carrying ALT,
 * one whose consensus carries REF has CR reads carrying REF.
 * sp_cyp_variant_windows (host only): the window of every variant on ONE consensus.  aln / cigar / n_cigar: the alignment of that consensus (query a) onto the backbone
 * (target b) from sp_affine_align_batch; var_pos: positions on the backbone (sp_cyp_problem.var_pos), var_ref_len: the lengths of REF.  Variant v with the backbone
 * interval [p - flank, p + |ref| + flank) is covered iff b_start <= p - flank and p + |ref| + flank <= b_end; a covered variant's window is [q_lo, q_hi): q_lo = the
 * query offset when the path has consumed the backbone up to p - flank, BEFORE any 'I' at that junction, q_hi = the query offset when it has consumed it up to
 * p + |ref| + flank, AFTER any 'I' at that junction -- inserted bases at the edges fall inside.  valid[v] = 1 and windows[v] set; 0 for a variant that is not covered or
 * whose window is empty (the whole interval under one 'D').  SP_ERR_INVALID_ARG for ops that do not consume the spans of aln.
 * SP_CYP_VCF_FLANK: the default flank, a design choice and not a measurement -- the smallest that puts the junction of a pure insertion (|ref| 0, or 1 after
 * normalisation) strictly inside its window and keeps one neighbouring base on each side beyond that.
 * sp_cyp_variant_support(_cohort): the driver -- call / consensus / cons_cap / mappings as sp_cyp_consensus_support takes them, problem and region_variants as
 * sp_cyp_diplotype_mappings took and returned them (_cohort: one sp_cyp_region_variants per sample).  Every has_variants consensus is aligned onto problem->backbone (one
 * sp_anchor_batch for the diagonals, one sp_affine_align_batch at the map-hifi scores on 256 diagonals), the windows are made by the rule above, and the member pass
 * of sp_cyp_consensus_support runs with them attached (sp_align_pileup_windows_batch).  support / support_valid: SP_CYP_MAXCONS * n_variants entries (per sample),
 * region h's at h * n_variants + v; support_valid 0 (and zero counts) where region h has no window for v.  col_offset / cols / cols_cap / summaries (optional, all or
 * none but cols): the table of sp_cyp_consensus_support from the SAME member pass.
 * sp_cyp_alleles_vcf (host only): the text.  support / support_valid (optional) as above: FORMAT becomes GT:SR:CR, with '.' for both where support_valid is 0; without
 * support FORMAT is GT alone and the records are the reference's, field for field.  file_date NULL: today (UTC, %Y%m%d); command NULL: "".  call->status != 0 or no typed
 * region: the header and the #CHROM line without samples, no records.  out / cap / needed as sp_cyp_alleles_json.
 * sp_bgzf_save: data as a BGZF file (gzip members with the 'BC' subfield of at most 64 KiB of input and 64 KiB as a block, raw deflate, the 28-byte EOF marker last).
 * sp_cyp_alleles_vcf_save: the text saved that way. */
#define SP_CYP_VCF_FLANK 2
int32_t sp_cyp_variant_windows(const sp_affine_aln* aln, const uint32_t* cigar, uint32_t n_cigar, uint32_t n_variants, const int32_t* var_pos, const uint32_t* var_ref_len,
                               uint32_t flank, sp_window* windows, int32_t* valid);
int32_t sp_cyp_variant_support(sp_ctx* ctx, const sp_cyp_problem* problem, const sp_seqset* reads, const sp_cyp_call* call, const char* consensus, uint32_t cons_cap,
                               const sp_cyp_region_variants* region_variants, const sp_cyp_read_mapping* mappings, uint64_t n_mappings, uint32_t flank,
                               sp_window_support* support, int32_t* support_valid, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap, sp_support_summary* summaries);
int32_t sp_cyp_variant_support_cohort(sp_ctx* ctx, const sp_cyp_problem* problem, uint32_t n_samples, const sp_seqset* const* reads, const sp_cyp_call* calls, const char* consensus,
                                      uint32_t cons_cap, const sp_cyp_region_variants* region_variants, const sp_cyp_read_mapping* mappings, const uint64_t* mapping_off, uint32_t flank,
                                      sp_window_support* support, int32_t* support_valid, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap, sp_support_summary* summaries);
typedef struct sp_cyp_db sp_cyp_db;            /* the CYP2D6 database, below */
int32_t sp_cyp_alleles_vcf(const sp_cyp_db* db, const sp_cyp_call* call, const sp_cyp_region_variants* region_variants, const sp_window_support* support /* optional */,
                           const int32_t* support_valid /* optional */, const char* file_date /* NULL: today, UTC, %Y%m%d */, const char* command /* NULL: "" */,
                           char* out, uint64_t cap, uint64_t* needed);
int32_t sp_cyp_alleles_vcf_save(const sp_cyp_db* db, const sp_cyp_call* call, const sp_cyp_region_variants* region_variants, const sp_window_support* support,
                                const int32_t* support_valid, const char* file_date, const char* command, const char* path);
int32_t sp_bgzf_save(const char* path, const void* data, uint64_t len);

/* ------------------------------------------------------------------ CYP2D6 templates and typing tables
 * Replaces generate_cyp_hybrids (src/cyp2d6/definitions.rs:346-464), LoadedVariants::load_variant_database
 * (src/cyp2d6/haplotyper.rs:650-773) and the table building of Cyp2d6Extractor::new (src/cyp2d6/haplotyper.rs:45-132).
 *   sp_cyp_locus     Cyp2d6Config::{cyp_coordinates, cyp_regions, cyp2d6_star5_del} (definitions.rs:17-30) as 0-based half-open
 *                    chromosome coordinates, plus the chromosome bases of a window that contains all of them (the reference reads
 *                    them with ReferenceGenome::get_slice); exon arrays hold exon1..exon9 of CYP2D6 / CYP2D7
 *   sp_cyp_gene_def  PgxDatabase::cyp2d6_gene_def (src/database/pgx_database.rs:41; AlleleDefinition / VariantDefinition,
 *                    src/data_types/alleles.rs:7-81) flattened in key (BTreeMap) order: allele a owns variants
 *                    [var_off[a], var_off[a+1]); var_id[x] == NULL means Option::None (the label becomes variant_string()),
 *                    var_vi[x] == NULL means no "VI" entry in extras
 *   sp_cyp_config    Cyp2d6Config::{cyp_translate, inferred_connections, unexpected_singletons} (definitions.rs:242-301)
 * Built: the 39 search templates in the visiting order of find_base_type_in_sequence (sorted by full_allele(),
 * haplotyper.rs:175-183) with type, subtype label and deep-typing flag (mapped_hybrids, :117-123); the ordered variant table
 * (first occurrence per (position, ref, alt), stable sort by position), labels, VI flags, label and variant look-ups; one 0/1 row per
 * star allele in haplotype_lookup (BTreeMap<Cyp2d6RegionLabel, _>) order.  ctx may be NULL: the tables are then host only
 * (sp_cyp_db_problem needs a context: it hands out the templates as a packed set in HBM).
 * Errors: SP_ERR_INVALID_ARG when a coordinate leaves the window, the CYP2D6 region does not contain every variant (the reference
 * asserts, haplotyper.rs:110-111) or a variant leaves the backbone. */
typedef struct {
    const char* chrom_name;                       /* "chr22" (used for variant_string() labels); NULL = "chr22" */
    const char* chrom_seq; uint64_t window_start, window_len;
    uint64_t d6_start, d6_end, d7_start, d7_end, rep6_start, rep6_end, rep7_start, rep7_end;
    uint64_t spacer_start, spacer_end, link_start, link_end, backbone_start, backbone_end, star5_start, star5_end;
    uint64_t d6_exon_start[9], d6_exon_end[9], d7_exon_start[9], d7_exon_end[9];
} sp_cyp_locus;
typedef struct {
    uint32_t n_alleles;
    const char* const* star_allele;               /* "4.001" */
    const uint32_t* var_off;                      /* n_alleles + 1 */
    const uint64_t* var_pos;                      /* 0-based on the chromosome */
    const char* const* var_ref; const char* const* var_alt;
    const char* const* var_id; const char* const* var_vi;     /* either array may be NULL altogether */
} sp_cyp_gene_def;
typedef struct {
    uint32_t n_translate; const char* const* translate_key; const char* const* translate_val;
    uint32_t n_connections; const char* const* connection_a; const char* const* connection_b;
    uint32_t n_singletons; const char* const* singletons;
} sp_cyp_config;
typedef struct {
    uint32_t n_templates, n_variants, n_vi, n_alleles, backbone_len;
    int64_t first_variant_pos, last_variant_pos;  /* LoadedVariants::{first,last}_variant_pos, -1 when there is none */
} sp_cyp_db_stats;
int32_t sp_cyp_db_create(sp_ctx* ctx /* may be NULL */, const sp_cyp_locus* locus, const sp_cyp_gene_def* gene_def, const sp_cyp_config* config /* may be NULL */,
                         sp_cyp_db** out);
void    sp_cyp_db_free(sp_cyp_db* db);
int32_t sp_cyp_db_info(const sp_cyp_db* db, sp_cyp_db_stats* stats);
/* the pointers stay valid for the life of the database; subtype is NULL for a label without one */
int32_t sp_cyp_db_template(const sp_cyp_db* db, uint32_t i, int32_t* type, const char** subtype, const char** full_allele, const char** seq, uint32_t* len, int32_t* deep);
int32_t sp_cyp_db_variant(const sp_cyp_db* db, uint32_t i, int64_t* chrom_pos, const char** ref, const char** alt, const char** label, int32_t* is_vi);
/* the "VI" entry of variant i as the database file has it (the last definition's, as LoadedVariants keeps it); *vi = NULL when the variant is not flagged.  Valid for
 * the life of the database. */
int32_t sp_cyp_db_variant_vi(const sp_cyp_db* db, uint32_t i, const char** vi);
int32_t sp_cyp_db_index_label(const sp_cyp_db* db, const char* label, uint32_t* idx);                                  /* LoadedVariants::index_label */
int32_t sp_cyp_db_index_variant(const sp_cyp_db* db, uint64_t position, const char* ref, const char* alt, uint32_t* idx);   /* LoadedVariants::index_variant */
int32_t sp_cyp_db_allele(const sp_cyp_db* db, uint32_t a, const char** subtype, const uint8_t** row /* n_variants 0/1 */);
/* everything sp_cyp_diplotype needs, pointing into the database (valid for its life); run parameters get the CLI defaults
 * (min_consensus_count 3, min_consensus_fraction 0.10, dual_max_ed_delta 100, no inferred connections, all alleles normalise) */
int32_t sp_cyp_db_problem(const sp_cyp_db* db, sp_cyp_problem* problem);

/* ------------------------------------------------------------------ K6: variant-gene diplotype search
 * Replaces solve_diplotype (src/diplotyper.rs:1211-1371) with find_best_inexact_matches (:1411-1509) and
 * NormalizedPgxHaplotype::quant_match (src/data_types/normalized_variant.rs:431-479) on integer ids.  The caller keeps the
 * string work (normalisation, names): variants are ids 0..n_vars-1, haplotypes are listed in defined_haplotypes (BTreeMap)
 * order, observed variants in BTreeMap<NormalizedVariant> order.
 *   haplotype h  = AND of slots [slot_off[h], slot_off[h+1]); slot s = OR of alt_var[alt_off[s] .. alt_off[s+1]) (-1 = None)
 *   obs_gt       SP_GT_* ; obs_ps = phase set or -1 ; obs_sv_label = -1 or the id of the SV haplotype label it carries
 * Every (het assignment, haplotype side, database haplotype) cell is scored on the GPU (one thread per cell); the host
 * combines the sides exactly as the reference does (ascending combinations, ties kept, sub-alleles shadow core alleles).
 * dip[i] = the two haplotype indices of diplotype i (an SV label l is encoded as -(l + 2)); dip_comb[i] = the het
 * assignment it came from (needed to derive the inexact haplotypes, :1516-1550). */
enum { SP_GT_HOM_REF = 0, SP_GT_HET_UNPHASED = 1, SP_GT_HET_PHASED = 2, SP_GT_HET_FLIP = 3, SP_GT_HOM_ALT = 4 };
#define SP_VAR_MAXDIP 4096

typedef struct {
    int32_t n_haps;
    const uint8_t* hap_is_sv;
    const uint8_t* hap_is_core;
    const int32_t* slot_off;
    const int32_t* alt_off;
    const int32_t* alt_var;
    int32_t n_vars;
    const uint8_t* var_is_core;
    int32_t n_obs;
    const int32_t* obs_var;
    const int32_t* obs_gt;
    const int64_t* obs_ps;
    const int32_t* obs_sv_label;
} sp_variant_problem;

typedef struct {
    int64_t score[4];                   /* core missing, core extra, sub missing, sub extra (INT64_MAX = unset) */
    int32_t n_dip, overflow;
    int32_t dip[SP_VAR_MAXDIP][2];
    int32_t dip_comb[SP_VAR_MAXDIP];
} sp_variant_result;

int32_t sp_variant_solve(sp_ctx* ctx, const sp_variant_problem* problem, sp_variant_result* result);
/* the solves of a panel / of one GPU's share of a cohort in one call, handed out to the context's streams (sp_ctx_set_option):
 * results[i] and problem_rc[i] (optional) are what sp_variant_solve gives for problems[i]; returns the first status that is not SP_OK */
int32_t sp_variant_solve_batch(sp_ctx* ctx, uint32_t n, const sp_variant_problem* const* problems, sp_variant_result* results, int32_t* problem_rc);

/* The runner-up diplotypes: what solve_diplotype prints of every combination at debug level and throws away (src/diplotyper.rs:1263-1357).
 * For a problem as sp_variant_solve takes it a CANDIDATE is (comb, dip0, dip1): comb a het assignment, 0 <= comb < n_comb (2^(groups - 1); 1 without
 * het calls), dip0 an explanation of side 0 and dip1 one of side 1.
 *   - A side that carries an SV label (obs_sv_label >= 0 on one of its members -- the homozygous calls first, then the side's het calls, each in call
 *     order) has exactly one explanation, -(first label + 2), with the side score (0, number of distinct labels among the remaining labelled
 *     members, 0, 0): the short-circuit of find_best_inexact_matches (:1414-1431).
 *   - Any other side is explained by every haplotype h that is not an SV haplotype and has core missing <= 1 (the reference's (1, MAX, MAX, MAX)
 *     bound); the side score is the cell's (core missing, core extra, sub missing, sub extra), the number the solve computes.  A side with no
 *     such haplotype makes its assignment contribute no candidate.
 *   - A problem without het calls has one side: its candidates are (0, h, h) and the total is that one side score, not doubled (:1239-1250);
 *     side_score[1] repeats side_score[0].  Otherwise the total is the component-wise sum of the two side scores.
 *   - There is no sub-allele shadowing: a core allele tied with a sub-allele on its side is a candidate like any other; SP_VAR_ALT_SHADOWED says
 *     that the reference's call drops it.
 *   - The list is ordered by (total score lexicographically, comb, dip0, dip1) ascending, dip compared as the signed value: a strict total order,
 *     so the n_best (1..64) first candidates are unique; they do not depend on the launch shape, the stream count or the position in a batch.
 * alts: n_best records; info->n_alts = min(n_best, candidates) are filled, the others are zero.  info->n_candidates: the sum over the assignments of
 * eligible explanations of side 0 x side 1.  info->best_score: the score sp_variant_solve reports -- entry 0's total whenever the solve lists a
 * diplotype, (core missing, MAX, MAX, MAX) when the smallest total belongs to an assignment with a side nothing explains (the solve then lists no
 * diplotype and n_called is 0, though candidates may exist: solve_diplotype compares such a total like any other, :1319-1357).  info->n_called: the
 * candidates at best_score that the reference's call keeps, i.e. sp_variant_solve's n_dip without its SP_VAR_MAXDIP bound.  Limits and statuses are
 * those of the solve (64 observations, 64 slots per haplotype, 24 groups); the batch form reports a failing problem in problem_rc (optional),
 * leaves its records zero, runs the others and returns the first status that is not SP_OK.  All problems of a batch run in one launch pair; device
 * memory is the tables plus workgroups x n_best records, pooled, whatever n_comb is.  The grid: with P problems in the launch, a problem runs on
 * min(n_comb, max(1, 8 * CUs / P)) one-wave workgroups (CUs: sp_ctx_get_info), each taking every wg_count-th assignment; the profile entry "k6_alt" counts
 * them as its cells. */
typedef struct { int64_t score[4]; int32_t side_score[2][4]; int32_t dip[2]; int32_t comb; uint32_t flags; } sp_variant_alt;
typedef struct { uint64_t n_comb, n_candidates; int64_t best_score[4]; uint32_t n_alts, n_called; } sp_variant_alt_info;
#define SP_VAR_ALT_CALLED   1u   /* (dip, comb) is one of sp_variant_solve's diplotypes */
#define SP_VAR_ALT_SHADOWED 2u   /* at the best total, but dropped from the call: a core allele tied with a sub-allele on its side */
#define SP_VAR_ALTERNATIVES 10   /* what the whole-sample switch asks for */
int32_t sp_variant_alternatives(sp_ctx* ctx, const sp_variant_problem* problem, uint32_t n_best, sp_variant_alt* alts, sp_variant_alt_info* info);
int32_t sp_variant_alternatives_batch(sp_ctx* ctx, uint32_t n, const sp_variant_problem* const* problems, uint32_t n_best, sp_variant_alt* alts /* n * n_best */,
                                      sp_variant_alt_info* infos, int32_t* problem_rc);
/* host only: the variants of side `side` (0 / 1) of het assignment comb under explanation dip, as the inexact haplotypes of the call name them
 * (het_split + quant_match, :1516-1550): the matching ids (SP_REL_MATCH), then the haplotype's unmatched variants (SP_REL_MISSING), then the side's
 * unexplained ones (SP_REL_UNEXPECTED).  Their MISSING / UNEXPECTED counts, split by var_is_core, are the record's side_score.  dip < 0 (an SV label):
 * the member that carries the label (MATCH) and the first member of every distinct label behind it (UNEXPECTED).  *n is always set (0 on
 * SP_ERR_INVALID_ARG); SP_ERR_CAPACITY when cap < *n; SP_ERR_INVALID_ARG for a side other than 0 / 1, a comb outside 0 .. n_comb - 1, a dip >= n_haps and an SV
 * label that is not the first one the side carries.  Any haplotype 0 .. n_haps - 1 is answered, also one the search does not list (an SV haplotype, core
 * missing > 1). */
int32_t sp_variant_alt_relations(const sp_variant_problem* problem, int32_t comb, int32_t side, int32_t dip, int32_t* ids, int32_t* rel, uint32_t cap, uint32_t* n);
/* host only: the text of one gene's entry of variant_alternatives.json: {"n_combinations", "n_candidates", "best_score", "alternatives": [...]}, best
 * first; an alternative has rank (1: the best), diplotype ("a/b" as the main call would spell this candidate: haplotype names for a score of
 * (0, 0, 0, 0), core allele names for (0, 0, ., .), NO_MATCH/NO_MATCH otherwise), called, shadowed, score {core_missing, core_unexpected,
 * sub_missing, sub_unexpected} (null: unset), combination, hap1 / hap2 {haplotype, score, missing, unexpected} with the variant names of
 * sp_variant_alt_relations.  Names come from the caller: hap_names / hap_core_names [n_haps] (the core allele of a sub-allele, its own name for a
 * core allele), sv_labels [n_sv_labels] (obs_sv_label ids), var_names [n_vars].  out / cap / needed as sp_cyp_alleles_json. */
int32_t sp_variant_alternatives_json(const sp_variant_problem* problem, const sp_variant_alt_info* info, const sp_variant_alt* alts, const char* const* hap_names,
                                     const char* const* hap_core_names, const char* const* sv_labels, uint32_t n_sv_labels, const char* const* var_names,
                                     char* out, uint64_t cap, uint64_t* needed);

/* is_deletion (src/diplotyper.rs:1020-1174): which defined deletion haplotype, if any, a deleted region [start, end) (0-based,
 * end exclusive) is; its label is what load_sv_vcf_variants (:739-857) attaches to the observed SV (obs_sv_label above).
 * Full-gene deletions are tried first (is_full_deletion, :1034-1089: a gene counts when its coordinates lie inside the region),
 * then partial ones (is_partial_deletion, :1098-1174: the first..last exon inside the region, indices mirrored on the reverse
 * strand).  Within a class the definitions are walked in the order given -- the caller lists them in label (BTreeMap) order
 * -- a generic definition matches when its genes are all among the deleted ones and is kept until a later one matches, a
 * specific definition needs the exact set (genes, and exon ranges for partial ones) and ends the walk.
 *   genes g = 0..n_genes-1: gene_start/gene_end, gene_forward, exons [exon_off[g], exon_off[g+1]) in reference order
 *   full definition d: genes full_gene[full_off[d] .. full_off[d+1])
 *   partial definition d: entries [partial_off[d], partial_off[d+1]) = (partial_gene, exons partial_first .. partial_end exclusive)
 *   a gene id of -1 = a gene without a definition in the gene collection -> SP_ERR_BAD_ARG (the reference bails, :1042-1046)
 * kind: 0 no match, 1 full deletion, 2 partial deletion; index: the matching definition within its class. */
typedef struct {
    int32_t n_genes;
    const int64_t* gene_start;
    const int64_t* gene_end;
    const uint8_t* gene_forward;
    const int32_t* exon_off;
    const int64_t* exon_start;
    const int64_t* exon_end;
    int32_t n_full;
    const uint8_t* full_generic;
    const int32_t* full_off;
    const int32_t* full_gene;
    int32_t n_partial;
    const uint8_t* partial_generic;
    const int32_t* partial_off;
    const int32_t* partial_gene;
    const int32_t* partial_first;
    const int32_t* partial_end;
} sp_sv_definitions;

int32_t sp_variant_is_deletion(const sp_sv_definitions* defs, uint64_t start, uint64_t end, int32_t* kind, int32_t* index);

/* ------------------------------------------------------------------ K8: read consensus by dynamic wavefront alignment
 * Serves the waffle_con calls of the reference: DualConsensusDWFA::{add_sequence_offset, consensus} in
 * run_dual_consensus_with_offsets (src/hla/caller.rs:1103-1219) and ConsensusDWFA per read group (src/hla/caller.rs:706-747),
 * with the fields of dwfa_config_from_cli (src/hla/caller.rs:1103-1116).  waffle_con v0.4.4 is not on disk: the contract is the
 * one in DESIGN.md section 9 / oracle/consensus.c (every read keeps a 64-diagonal edit wavefront against the growing consensus
 * and votes for the next base; extensions are explored best first -- lowest total edit distance, then longest -- under the bounds
 * max_queue_size / max_capacity_per_size / max_nodes_wo_constraint; a candidate needs min_count reads and min_af of the votes;
 * a pair of candidates may start a second consensus).
 *   reads / read_idx   the sequences (read_idx == NULL: all n = sp_seqset_count(reads) of them, in order)
 *   offsets            NULL, or per sequence -1 (None: starts with the consensus) or the consensus length at which the sequence is
 *                      placed; its start is searched in the offset_window bases before that point (add_sequence_offset)
 *   cons1 / cons2      cap bytes each, NUL terminated ASCII; cons2 is empty unless result->is_dual
 *   is_cons1, score1, score2   DualConsensus::{is_consensus1, scores1, scores2}; a score of -1 is None
 * sp_consensus runs the search with cfg->allow_dual as given (ConsensusDWFA / DualConsensusDWFA); sp_consensus_dual is the same
 * with a second consensus allowed. */
typedef struct {
    int32_t min_count;                 /* 3 */
    int32_t dual_max_ed_delta;         /* 100 */
    int32_t allow_early_termination;
    int32_t allow_dual;
    int32_t offset_window;             /* 400 */
    int32_t offset_compare_length;     /* 50 for HLA (src/hla/caller.rs:1114), 100 for CYP2D6 (src/cyp2d6/caller.rs:144).  At most 128; at most 64 when offset_window + offset_compare_length exceeds 512.
                                        * A read with an offset is placed when the consensus reaches offset + min(offset_compare_length, its length): its start is searched in
                                        * [offset - offset_window, offset], its first bases compared with the consensus behind each start (free end on the consensus) */
    double  min_af;                    /* 0.10 */
    int32_t max_queue_size;            /* 20    CdwfaConfig::max_queue_size, set by dwfa_config_from_cli (src/hla/caller.rs:1110) */
    int32_t max_capacity_per_size;     /* 10    CdwfaConfig::max_capacity_per_size (:1111) */
    int32_t max_nodes_wo_constraint;   /* 1000  waffle_con's default; the reference does not set it */
    int32_t no_retry_ladder;           /* (<= 0 in any of the three above: the value named there)  sp_consensus_priority only: 1 = a two-way search that
                                        * gives up is NOT run again with stricter fractions (see there); sp_cyp_diplotype* set it unless the context's "cons_retry_ladder" is 1 */
} sp_cons_config;

typedef struct {
    int32_t is_dual, len1, len2, split_at;
    int64_t gave_up, best_total;       /* gave_up = 1: the search ended without a complete node (its bounds exhausted): no consensus, every read in group 1 */
    int64_t split_w2, split_total;     /* (best_total and this pair are unused since the best-first search replaced the two-pass split policy) */
    int64_t nodes_expanded;            /* nodes the search took out of its queue and expanded */
} sp_cons_result;

/* batched form: independent problems advance in lockstep (one base per kernel launch for all of them), so a batch costs as many
 * launches as its longest consensus.  outputs[p].status is SP_OK or SP_ERR_CAPACITY (cap too small for that consensus). */
typedef struct {
    const sp_seqset* reads; const uint32_t* read_idx; uint32_t n; const int32_t* offsets;
    sp_cons_config cfg;
} sp_cons_problem;
typedef struct {
    char* cons1; char* cons2; uint32_t cap;
    uint8_t* is_cons1; int32_t* score1; int32_t* score2;
    sp_cons_result result; int32_t status;
} sp_cons_output;
int32_t sp_consensus_batch(sp_ctx* ctx, uint32_t n_problems, const sp_cons_problem* problems, sp_cons_output* outputs);
int32_t sp_consensus_dual_batch(sp_ctx* ctx, uint32_t n_problems, const sp_cons_problem* problems, sp_cons_output* outputs);

int32_t sp_consensus(sp_ctx* ctx, const sp_seqset* reads, const uint32_t* read_idx, uint32_t n, const int32_t* offsets,
                     const sp_cons_config* cfg, char* cons1, char* cons2, uint32_t cap,
                     uint8_t* is_cons1, int32_t* score1, int32_t* score2, sp_cons_result* result);
int32_t sp_consensus_dual(sp_ctx* ctx, const sp_seqset* reads, const uint32_t* read_idx, uint32_t n, const int32_t* offsets,
                          const sp_cons_config* cfg, char* cons1, char* cons2, uint32_t cap,
                          uint8_t* is_cons1, int32_t* score1, int32_t* score2, sp_cons_result* result);

/* multi-way consensus by repeated two-way splits: the role of PriorityConsensusDWFA::{add_seeded_sequence_chain, consensus} in the
 * CYP2D6 caller (src/cyp2d6/caller.rs:162-270).  Every read contributes one sequence per level (the reference chains the
 * homopolymer-compressed segment, then the raw segment) with its own offset; seeds force an initial grouping (:231-238).
 * Contract: solve(group, level) = run sp_consensus_dual on the group's level sequences; if it splits, solve(consensus-1 reads,
 * level) followed by solve(the others, level); else solve(group, level + 1), or emit the group after the last level.  Initial
 * groups: the unseeded reads, then each seed in ascending order.  Offsets inside a group are re-based on the group's smallest
 * one (that read starts the consensus, the others keep their distance to it plus half the window).  Finally every emitted group
 * gets one consensus per level: the consensus its own two-way search at that level left when that search ended with ONE consensus at the configured
 * fraction (the search that found the group indivisible), otherwise (a group born from a split at a later level, a search that gave up or was retried) a
 * search of its own (sp_consensus).  All problems of a round run in lockstep on the GPU.  A two-way search that gives up (no
 * complete node: a group of more classes than a search holds consensuses can exhaust the queue / capacity bounds at high depth) is run
 * again with min_af 0.15, 0.20, 0.30, 0.40 (the first above the configured one that completes); the groups it leaves are solved with the
 * configured fraction again.  This retry is a rule of this library, not of waffle_con: cfg.no_retry_ladder = 1 switches it off (the group then
 * stays whole, as a search that gives up leaves it).  "Gave up" is sp_cons_result.gave_up of the two-way search, not an empty string.
 *   levels[l]   the sequences of level l (n each, same read order); offsets[l] = NULL or n entries (-1 = None); seeds = NULL or n (-1 = None)
 *   group_of    n entries: index of the emitted group of every read (MultiConsensus::sequence_indices)
 *   cons        max_groups * n_levels * cap bytes: consensus of group g at level l at cons + (g * n_levels + l) * cap
 * Returns SP_ERR_CAPACITY when there are more than max_groups groups (n_groups then holds the number needed). */
typedef struct {
    uint32_t n_levels, n;
    const sp_seqset* const* levels;
    const int32_t* const* offsets;
    const int32_t* seeds;
    sp_cons_config cfg;
} sp_priority_problem;
int32_t sp_consensus_priority(sp_ctx* ctx, const sp_priority_problem* problem, uint32_t max_groups, uint32_t cap,
                              uint32_t* n_groups, int32_t* group_of, char* cons);

/* Several multi-way consensus problems (the samples of a cohort) in lockstep: what sp_consensus_priority does for each, with all open groups of all
 * problems of a round in the same launches.  status: SP_OK, or why this job alone could not be solved (SP_ERR_CAPACITY: more groups than max_groups). */
typedef struct sp_priority_job {
    const sp_priority_problem* problem;
    uint32_t max_groups, cap;
    uint32_t* n_groups; int32_t* group_of; char* cons;      /* as the arguments of sp_consensus_priority */
    int32_t status;
    int32_t gave_up;                                        /* out: two-way searches of this job that ended without a complete node (sp_cons_result.gave_up) and were not retried */
} sp_priority_job;
int32_t sp_consensus_priority_many(sp_ctx* ctx, uint32_t n_jobs, sp_priority_job* jobs);

/* ------------------------------------------------------------------ one HLA gene, reads to diplotype
 * The gene loop of diplotype_hla_batch (src/hla/caller.rs:642-1040) on top of K1 / K8 / K2, without I/O and debug artefacts:
 * the realigned segments of `gene` (realign[r].status == 0, in input order = qname order) are cut out of the packed reads and
 * homopolymer-compressed on the device; run_dual_consensus_with_offsets (:1118-1219: HPC first, DNA if is_passing_dual fails);
 * is_hemizygous_better when the gene is absent-capable (:676-684); one consensus per read group (:706-747); score_consensus on
 * each (:756,829); heterozygous if the dual passes, else homozygous for the larger group (:889-912).
 *   realign      the K1 output for `reads` (sp_hla_realign_reads)
 *   cons1/cons2  cap bytes each: the hg38-forward consensus of each group (empty = none / failed)
 *   is_cons1     optional, one entry per read of `reads`: DualConsensus::is_consensus1 (0 for reads not realigned to the gene)
 * call->status: 0 = called, 1 = no realigned reads (NO_READS / NO_CALL, :662-668).  allele1/allele2 are database indices,
 * -1 = unknown (no allele typed), -2 = the absent haplotype of a hemizygous call (:919-923). */
typedef struct {
    int32_t min_consensus_count;       /* --min-consensus-count (3) */
    int32_t dual_max_ed_delta;         /* --dual-max-ed-delta (100) */
    double  min_consensus_fraction;    /* --min-consensus-fraction (0.10) */
    double  expected_maf, min_cdf;     /* is_passing_dual (src/hla/caller.rs:1225-1247) */
    int32_t require_dna, disable_cdna; /* --hla-require-dna, --disable-cdna-scoring */
    int32_t absent_capable;            /* gene_def.is_absent_capable() */
    double  normalized_coverage;       /* < 0: unknown */
} sp_hla_call_config;

typedef struct {
    int32_t status;
    int32_t allele1, allele2;
    int32_t typed1, typed2;            /* best database allele of each consensus (-1 = none) */
    int32_t n_reads, counts1, counts2;
    int32_t is_dual, dual_passed, is_hemizygous, used_dna_dual;
    int32_t cons1_len, cons2_len;
    double  maf, cdf;
} sp_hla_call;

int32_t sp_hla_diplotype_gene(sp_ctx* ctx, const sp_hla_db* db, uint32_t gene, const sp_seqset* reads, const sp_hla_realign* realign,
                              const sp_hla_call_config* cfg, sp_hla_call* call, char* cons1, char* cons2, uint32_t cap, uint8_t* is_cons1);
/* several genes at once: their consensus problems advance in lockstep on the GPU (the gene buckets are independent,
 * src/hla/caller.rs:642), so the whole sample costs as many launches as its longest gene.  cfgs / calls: n_genes entries;
 * cons: n_genes * 2 * cap bytes, consensus c of gene k at cons + (2k + c) * cap. */
int32_t sp_hla_diplotype_genes(sp_ctx* ctx, const sp_hla_db* db, uint32_t n_genes, const uint32_t* genes, const sp_seqset* reads,
                               const sp_hla_realign* realign, const sp_hla_call_config* cfgs, sp_hla_call* calls,
                               char* cons, uint32_t cap, uint8_t* is_cons1);
/* a cohort at once: `reads` holds the reads of n_samples samples (read_sample[r] = sample of read r; one sp_hla_realign_reads call
 * serves them all), and the consensus problems of every (sample, gene) advance in lockstep -- for WGS-sized samples a launch costs
 * the same whether it serves one sample or dozens.  cfgs: n_genes entries; calls: n_samples * n_genes, sample-major;
 * cons: n_samples * n_genes * 2 * cap bytes, laid out like calls. */
int32_t sp_hla_diplotype_cohort(sp_ctx* ctx, const sp_hla_db* db, uint32_t n_samples, const uint32_t* read_sample, uint32_t n_genes, const uint32_t* genes,
                                const sp_seqset* reads, const sp_hla_realign* realign, const sp_hla_call_config* cfgs, sp_hla_call* calls,
                                char* cons, uint32_t cap, uint8_t* is_cons1);
/* the same with a configuration per (sample, gene): cfgs has n_samples * n_genes entries, sample-major like calls.  A cohort of files needs it:
 * normalized_coverage (sp_hla_normalized_coverage over the sample's own HLA-DRB1 records) differs from sample to sample. */
int32_t sp_hla_diplotype_cohort_samples(sp_ctx* ctx, const sp_hla_db* db, uint32_t n_samples, const uint32_t* read_sample, uint32_t n_genes, const uint32_t* genes,
                                        const sp_seqset* reads, const sp_hla_realign* realign, const sp_hla_call_config* cfgs, sp_hla_call* calls,
                                        char* cons, uint32_t cap, uint8_t* is_cons1);

/* ------------------------------------------------------------------ consensus support: how well the member reads back each consensus of a gene call
 * An output of this library's own (the reference has no such table: its users open debug_consensus.bam in IGV and look at the pile of reads under each consensus base;
 * this hands out the integers they read off that picture, not the picture).  Arguments as sp_hla_diplotype_gene took and returned them.  Members of consensus 1 / 2 are
 * the realigned reads of the gene (realign[r].status == 0 and .gene == gene) with is_cons1[r] != 0 / == 0.  Query: the read's DNA segment [seg_start, seg_end), the one
 * the group consensus was built from, put on the gene strand (reverse-complemented for a reverse-strand gene).  Target: the gene-strand DNA consensus (cons as given
 * for a forward gene, its reverse complement otherwise: sp_hla_map_consensus_seq's level 1).  Alignment: sp_affine_align_batch at the map-hifi scores {1, 4, 6, 2, 26,
 * 1, 1} on the diagonal the anchor gives -- sp_anchor_batch(A = the consensuses, B = the segments) votes for (segment position - consensus position), the pair's diag
 * is its negation -- on 64 diagonals, and once more on 256 when that found nothing (score 0).  A member without an anchor (0 votes) or without an alignment on either
 * band is counted in n_unaligned and left out; it is not an error.  cols1 / cols2: strlen(cons1) / strlen(cons2) columns of sp_pileup_batch over the aligned members
 * (gene-strand coordinates); an empty consensus gets a zeroed summary.  Either pair of outputs may be NULL.
 * sp_support_summary: length = columns; min_depth and median_depth (the lower median: element (length - 1) / 2 of the sorted depths) over all columns; n_contested
 * columns are contested: 2 * eq <= depth with depth > 0 (the consensus base lacks a strict majority of the spanning members) or 2 * ins > depth (an insertion
 * behind the column has one).  The rule has no parameter.  sp_support_summarize / sp_support_contested apply it to any table (host only).
 * sp_hla_consensus_support_cohort: every (sample, gene) unit of sp_hla_diplotype_cohort_samples in one pass -- one segment set, one anchor launch, one alignment
 * launch per band, one pileup launch.  cons / is_cons1 as that call returned them; read_sample NULL = one sample.  unit_on (optional, n_samples * n_genes): 0 skips a
 * unit (its consensuses get no columns and zeroed summaries).  col_offset (n_samples * n_genes * 2 + 1 entries, always filled): consensus c of unit u owns
 * cols[col_offset[2u + c] .. col_offset[2u + c + 1]); SP_ERR_CAPACITY when col_offset[last] > cols_cap (nothing else is written: call again with more room).
 * summaries: n_samples * n_genes * 2.  (sp_support_summary: declared with sp_align_pileup_batch above, 32 bytes.) */
int32_t sp_support_summarize(const sp_pileup_col* cols, uint32_t length, uint32_t n_members, uint32_t n_aligned, sp_support_summary* out);
/* the contested columns in ascending order: pos holds cap entries, *n = how many there are (SP_ERR_CAPACITY when more than cap) */
int32_t sp_support_contested(const sp_pileup_col* cols, uint32_t length, uint32_t* pos, uint32_t cap, uint32_t* n);
int32_t sp_hla_consensus_support(sp_ctx* ctx, const sp_hla_db* db, uint32_t gene, const sp_seqset* reads, const sp_hla_realign* realign, const uint8_t* is_cons1,
                                 const char* cons1, const char* cons2, sp_pileup_col* cols1, sp_pileup_col* cols2, sp_support_summary* s1, sp_support_summary* s2);
int32_t sp_hla_consensus_support_cohort(sp_ctx* ctx, const sp_hla_db* db, uint32_t n_samples, const uint32_t* read_sample, uint32_t n_genes, const uint32_t* genes,
                                        const sp_seqset* reads, const sp_hla_realign* realign, const uint8_t* is_cons1, const char* cons, uint32_t cap,
                                        const uint8_t* unit_on, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap, sp_support_summary* summaries);
/* `consensus_support.json` (host only; the layout of the other debug files: two-space indent).  One entry per gene; the file is keyed by gene in name order, then by
 * "consensus1" / "consensus2" (a consensus whose `consensus` is NULL or empty is left out, a gene with neither is omitted).  Each holds n_members, n_aligned,
 * n_unaligned, length, min_depth, median_depth, n_contested, typed_allele (NULL: null) and contested = [{pos, depth, eq, x: [a, c, g, t], del, ins, consensus_base}]
 * for the contested columns of cols (pos 0-based on the gene-strand consensus, consensus_base its letter).  The full table stays behind the API.
 * out / cap / needed as sp_cyp_alleles_json. */
typedef struct {
    const char* gene;
    const char* typed_allele[2];        /* the star string of the call for each consensus */
    const char* consensus[2];           /* gene-strand DNA consensus, NUL-terminated; its length must be summary[c]->length */
    const sp_pileup_col* cols[2];
    const sp_support_summary* summary[2];
} sp_support_entry;
int32_t sp_consensus_support_json(const sp_support_entry* entries, uint32_t n_entries, char* out, uint64_t cap, uint64_t* needed);
/* The support calls with the insertion list of sp_align_pileup_ins_batch (ins / ins_cap / n_ins as there; ins == NULL is the call without: nothing else is launched).
 * Same members, bands and retry rule.  col: sp_hla_consensus_support_ins numbers consensus 1's columns from 0 and consensus 2's from strlen(cons1) (only the
 * consensuses whose outputs are given take part); the cohort form uses its col_offset.  Strings and positions are on the gene strand, as the columns are.  first_pair
 * is the index of the member READ in `reads`, first_qpos the run's position in the member's gene-strand segment.
 * sp_consensus_support_json_ins: sp_consensus_support_json with a list.  col_base: 2 per entry, the col of column 0 of consensus c of entry e at col_base[2 e + c]
 * (not read, and may be NULL, when there are no entries: the text is {} whatever the list holds -- a list may be a whole batch group's).
 * Every contested entry with 2 * ins > depth gains
 *     "insertions": [{"seq": "...", "count": n}, ...], "other": n_other
 * -- the column's records with len > 0 in record order, at most 8 ("more": the number left out, only when there are any); a string of more than 64 bases is written
 * as its first 64 with "len": L behind count; "first_read": the QNAME, behind those, when read_names (n_read_names entries, indexed by first_pair) is given; "other" only
 * when n_other > 0.  ins == NULL or n_ins == 0: the bytes of sp_consensus_support_json. */
int32_t sp_hla_consensus_support_ins(sp_ctx* ctx, const sp_hla_db* db, uint32_t gene, const sp_seqset* reads, const sp_hla_realign* realign, const uint8_t* is_cons1,
                                     const char* cons1, const char* cons2, sp_pileup_col* cols1, sp_pileup_col* cols2, sp_support_summary* s1, sp_support_summary* s2,
                                     sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins);
int32_t sp_hla_consensus_support_cohort_ins(sp_ctx* ctx, const sp_hla_db* db, uint32_t n_samples, const uint32_t* read_sample, uint32_t n_genes, const uint32_t* genes,
                                            const sp_seqset* reads, const sp_hla_realign* realign, const uint8_t* is_cons1, const char* cons, uint32_t cap,
                                            const uint8_t* unit_on, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap, sp_support_summary* summaries,
                                            sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins);
int32_t sp_consensus_support_json_ins(const sp_support_entry* entries, uint32_t n_entries, const uint64_t* col_base, const sp_pileup_ins* ins, uint64_t n_ins,
                                      const char* const* read_names, uint32_t n_read_names, char* out, uint64_t cap, uint64_t* needed);
/* The _ins forms with the haplotype list of sp_align_pileup_hap_batch as well (haps / hap_cap / n_haps / heads as there; haps == NULL is the _ins form: nothing else is
 * launched).  target is numbered as the columns are: sp_hla_consensus_support_hap gives consensus 1 target 0 and consensus 2 target 1 (heads: 2); the cohort form uses the
 * slot of its col_offset, 2 * unit + consensus (heads: one per slot, an unused slot's is empty).  first_pair is the index of the member READ in `reads`.  Calls are on the
 * gene strand, as the columns are.  Either list may be asked for without the other; SP_ERR_CAPACITY names the list that did not fit by its count, the other is complete.
 * sp_consensus_support_json_hap: sp_consensus_support_json_ins with a list.  hap_target: 2 per entry, the target of consensus c of entry e at hap_target[2 e + c];
 * heads: n_heads records indexed by target.  A consensus whose head has n_cols > 0 and records gains, behind "contested",
 *     "haplotypes": {"columns": [pos, ...], "columns_total": K', "patterns": [{"count": n, "calls": "...", "first_read": "QNAME"}, ...], "more": n}
 * -- columns: the n_cols used positions; patterns: the records in record order, at most 16, calls as sp_support_hap_string writes them; "more": the number of reads in
 * the patterns left out, only when there are any; "first_read" only when read_names (indexed by first_pair) is given.  haps == NULL or n_haps == 0: the bytes of
 * sp_consensus_support_json_ins. */
int32_t sp_hla_consensus_support_hap(sp_ctx* ctx, const sp_hla_db* db, uint32_t gene, const sp_seqset* reads, const sp_hla_realign* realign, const uint8_t* is_cons1,
                                     const char* cons1, const char* cons2, sp_pileup_col* cols1, sp_pileup_col* cols2, sp_support_summary* s1, sp_support_summary* s2,
                                     sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins, sp_support_hap* haps, uint64_t hap_cap, uint64_t* n_haps, sp_support_hap_head* heads);
int32_t sp_hla_consensus_support_cohort_hap(sp_ctx* ctx, const sp_hla_db* db, uint32_t n_samples, const uint32_t* read_sample, uint32_t n_genes, const uint32_t* genes,
                                            const sp_seqset* reads, const sp_hla_realign* realign, const uint8_t* is_cons1, const char* cons, uint32_t cap,
                                            const uint8_t* unit_on, uint64_t* col_offset, sp_pileup_col* cols, uint64_t cols_cap, sp_support_summary* summaries,
                                            sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins, sp_support_hap* haps, uint64_t hap_cap, uint64_t* n_haps, sp_support_hap_head* heads);
int32_t sp_consensus_support_json_hap(const sp_support_entry* entries, uint32_t n_entries, const uint64_t* col_base, const sp_pileup_ins* ins, uint64_t n_ins,
                                      const sp_support_hap* haps, uint64_t n_haps, const sp_support_hap_head* heads, uint64_t n_heads, const uint64_t* hap_target,
                                      const char* const* read_names, uint32_t n_read_names, char* out, uint64_t cap, uint64_t* needed);

/* ------------------------------------------------------------------ host-side decisions of the path (no device work)
 * Small scalar routines the reference evaluates between the kernels; kept behind the same ABI so a host can drop the whole
 * path in.  statrs 0.16 formulas (Binomial::cdf / ln_pmf, Normal::ln_pdf, ln_factorial). */
/* is_passing_dual (src/hla/caller.rs:1225-1247): returns 1 when maf >= min_consensus_fraction and Binomial(expected_maf, n).cdf(minor) >= min_cdf */
int32_t sp_hla_is_passing_dual(uint64_t counts1, uint64_t counts2, double min_consensus_fraction, double expected_maf, double min_cdf,
                               double* maf_out, double* cdf_out);
/* is_hemizygous_better (src/hla/caller.rs:1583-1653): scores1/scores2 < 0 mean None; normalized_coverage < 0 means unknown */
int32_t sp_hla_is_hemizygous_better(const int64_t* scores1, const int64_t* scores2, const uint8_t* is_consensus1, uint32_t n_reads,
                                    int32_t is_dual, uint64_t dual_max_ed_delta, double normalized_coverage,
                                    double* haploid_cost, double* diploid_cost);
/* the coverage normalisation of diplotype_hla_batch (src/hla/caller.rs:598-617): reads realigned to the normalising genes (NORMALIZING_HLA_GENES,
 * src/hla/alleles.rs:49-59: HLA-DRB1) over two haplotypes for each of those genes that has reads; *normalized_coverage = -1 (None) when none has --
 * the value sp_hla_call_config.normalized_coverage takes for the absent-capable genes (DRB3 / 4 / 5) */
int32_t sp_hla_normalized_coverage(const sp_hla_realign* realign, uint32_t n_reads, const uint32_t* normalizing_genes, uint32_t n_normalizing,
                                   double* normalized_coverage);
/* hpc_pos / hpc_bytes (src/util/homopolymers.rs:18-42) */
uint64_t sp_hpc_pos(const char* seq, uint64_t len, uint64_t position);
uint64_t sp_hpc(const char* seq, uint64_t len, char* out);
/* convert_chain_to_hap (src/cyp2d6/caller.rs:907-957); detail 0 = core alleles, 1 = sub-alleles; returns the string length
 * (the output is truncated to cap-1 characters) */
uint32_t sp_cyp_chain_to_hap(const int32_t* chain, uint32_t n, const int32_t* hap_type, const char* const* hap_subtype,
                             uint32_t n_translate, const char* const* translate_key, const char* const* translate_val,
                             int32_t detail, char* out, uint32_t cap);

/* NormalizedVariant::new (src/data_types/normalized_variant.rs:43-170) with parse_sequence (:262-279): CPIC allele syntax
 * ("del", "ins..", "delins..", "XYZ(n)"), anchor base, suffix / prefix trimming, left shift along the reference.
 * chrom_seq = the contig (NULL = no reference genome: no anchoring / shifting, as in the reference); position is 0-based.
 * out_ref / out_alt hold cap bytes each.  SP_ERR_BAD_VARIANT for every condition on which the reference bails. */
int32_t sp_variant_normalize(const char* chrom_seq, uint64_t chrom_len, uint64_t position, const char* ref_allele, const char* alt_allele,
                             uint64_t* out_position, char* out_ref, char* out_alt, uint32_t cap);
/* NormalizedVariant::multi_new (:174-214): IUPAC codes and "; " lists expand to several alternatives; is_none[i] = 1 where the
 * alternative equals the reference allele (Option::None).  Outputs are strided by cap; returns the count in n_out. */
int32_t sp_variant_multi_normalize(const char* chrom_seq, uint64_t chrom_len, uint64_t position, const char* ref_allele, const char* alt_allele,
                                   uint32_t max_out, uint32_t* n_out, uint8_t* is_none, uint64_t* out_position, char* out_ref, char* out_alt, uint32_t cap);

/* chain building between K4 and K5 (src/cyp2d6/caller.rs:429-583): per read, the cartesian product of the minimum-edit
 * consensuses of its kept segments (:461-491); best_allele_mapping_counts (:478-481); reads without a chain are dropped
 * (:494-517); chains that use a consensus nothing maps to uniquely are removed (:521-538) and those consensuses are flagged
 * for mark_false_allele() (:574-583).  Segments of read r = [read_seg_off[r], read_seg_off[r+1]); ed / kept as written by
 * sp_cyp_weight_segments.  Outputs feed sp_chain_problem directly:
 *   read_index[k] (k < info->n_reads)  input index of the k-th recorded read (input order = BTreeMap order of the caller)
 *   read_chain_off[n_reads+1], chain_off[chain_cap+1], chain_items[item_cap]   obs_chains
 *   read_w_off[n_reads+1], w_seg[n_segments]   chain_scores rows as segment indices into ed / ov
 *   unique_counts[n_haps], false_allele[n_haps]
 * Returns SP_OK, SP_ERR_CAPACITY (info holds the sizes needed) or SP_ERR_CHAIN_COLLAPSE. */
typedef struct { uint32_t n_reads, n_chains, n_items, n_rows; } sp_chain_build_info;
int32_t sp_cyp_build_chains(uint32_t n_haps, const int32_t* hap_type, uint32_t n_reads, const uint32_t* read_seg_off,
                            const uint64_t* ed, const uint8_t* kept,
                            uint32_t* read_index, uint32_t* read_chain_off, uint32_t* chain_off, uint32_t chain_cap,
                            uint32_t* chain_items, uint32_t item_cap, uint32_t* read_w_off, uint32_t* w_seg,
                            uint64_t* unique_counts, uint8_t* false_allele, sp_chain_build_info* info);

/* result strings (src/data_types/pgx_diplotype.rs, src/data_types/region_variants.rs) */
/* Diplotype::diplotype ("h1/h2", :13-20) or, pharmcat != 0, Diplotype::pharmcat_diplotype (haplotypes containing '+' in brackets, :51-64);
 * returns the string length (the output is truncated to cap-1 characters) */
uint32_t sp_diplotype_string(const char* hap1, const char* hap2, int32_t pharmcat, char* out, uint32_t cap);
/* InexactHaplotype::new + full_haplotype (:138-196): variants = RegionVariant{label, is_vi, state}, taken in BTreeSet order
 * (label, is_vi, state; duplicates collapse); every variant that is not a Match is appended as " <sign><label>" with the sign of
 * RegionVariant's Display ('+' Unexpected, '-' Missing, '?' the ambiguous / unknown states, region_variants.rs:44-60) and the
 * whole is put in parentheses; match_type: sub-allele match when all match, core match when every VI variant matches. */
enum { SP_REL_UNKNOWN = 0, SP_REL_MATCH = 1, SP_REL_UNEXPECTED = 2, SP_REL_MISSING = 3, SP_REL_AMBIGUOUS_UNEXPECTED = 4,
       SP_REL_AMBIGUOUS_MISSING = 5, SP_REL_UNKNOWN_UNEXPECTED = 6, SP_REL_UNKNOWN_MISSING = 7 };     /* VariantAlleleRelationship */
enum { SP_INEXACT_UNKNOWN = 0, SP_INEXACT_NO_MATCH = 1, SP_INEXACT_CORE_MATCH = 2, SP_INEXACT_SUBALLELE_MATCH = 3 };   /* InexactMatchType */
uint32_t sp_inexact_haplotype(const char* base_haplotype, uint32_t n_variants, const char* const* labels, const uint8_t* is_vi,
                              const int32_t* states, int32_t* match_type, char* out, uint32_t cap);

/* ------------------------------------------------------------------ f3: the database file and the result file (host only)
 * sp_database_* replaces the serde loading of PgxDatabase (src/database/pgx_database.rs:23-41; load_json, src/util/file_io.rs:16-28
 * -- gzip is recognised by its magic number here, not by the ".gz" extension) and the three flattenings the kernels' inputs need:
 * hla_sequences + hla_config -> sp_hla_db_desc (src/hla/alleles.rs:332-344; src/hla/realigner.rs:42-91), cyp2d6_config +
 * cyp2d6_gene_def -> sp_cyp_locus / sp_cyp_gene_def / sp_cyp_config, and one gene entry (PgxGene / PgxVariant / PgxHaplotype,
 * src/database/pgx_database.rs:373-840) -> sp_variant_gene -> sp_variant_problem.  Files written by older releases load too: a missing
 * "cyp2d6_config" / "hla_config" gets the reference's defaults, "hla_config" is read in its gene_collection form and in the older
 * hla_coordinates / hla_exons / hla_is_forward_strand form, is_core_variant / is_core_haplotype default to true.
 * Every pointer handed out belongs to the object it came from and stays valid until that object is freed (flatten results: until the
 * next flatten call of the same kind).  Errors: SP_ERR_INVALID_ARG, with the text in err / sp_database_last_error. */
typedef struct sp_database sp_database;
int32_t sp_database_load(const char* path, sp_database** out, char* err, uint32_t err_cap);                 /* .json or .json.gz */
int32_t sp_database_parse(const char* text, uint64_t len, sp_database** out, char* err, uint32_t err_cap);  /* JSON text or gzip bytes */
void    sp_database_free(sp_database* db);
const char* sp_database_last_error(const sp_database* db);
typedef struct {                                  /* PgxMetadata (src/database/pgx_database.rs:358-371) */
    const char* pbstarphase_version; const char* cpic_version; const char* hla_version; const char* pharmvar_version; const char* build_time;
} sp_database_metadata;
int32_t sp_database_get_metadata(const sp_database* db, sp_database_metadata* out);
typedef struct {
    uint32_t n_gene_entries, n_hla_sequences, n_hla_genes, n_cyp2d6_alleles, n_collection_genes;
    int32_t has_hla_config, has_cyp2d6_config, reserved;
} sp_database_stats;
int32_t sp_database_info(const sp_database* db, sp_database_stats* out);
typedef struct {                                  /* GeneDefinition (src/database/gene_definition.rs:18-34); 0-based half-open */
    const char* name; const char* chrom; uint64_t start, end;
    int32_t is_forward_strand, is_absent_capable; uint32_t n_exons, reserved;
    const uint64_t* exon_start; const uint64_t* exon_end;
} sp_gene_region;
int32_t sp_database_hla_gene(const sp_database* db, uint32_t g, sp_gene_region* out);         /* g < n_hla_genes, gene-name order */
int32_t sp_database_gene_entry(const sp_database* db, uint32_t i, const char** gene_name, const char** chromosome);   /* i < n_gene_entries */
/* the HLA part as sp_hla_db_create wants it.  gene_names: the genes to type, NULL = every gene of hla_config; gene_ref[g] = the hg38
 * bases of [start - ref_buffer, end + ref_buffer) of gene g; alleles of other genes are left out, the others keep database-key order */
int32_t sp_database_hla_flatten(sp_database* db, uint32_t n_genes, const char* const* gene_names, const char* const* gene_ref, int32_t ref_buffer,
                                sp_hla_db_desc* desc);
/* allele i of the last sp_database_hla_flatten: "HLA:HLA00001", "HLA-A", "01:01:01:01" */
int32_t sp_database_hla_allele(const sp_database* db, uint32_t i, const char** hla_id, const char** gene_name, const char** star_allele);
/* the smallest chromosome window holding every CYP2D6 coordinate of the configuration */
int32_t sp_database_cyp_window(const sp_database* db, const char** chrom, uint64_t* start, uint64_t* end);
/* the CYP2D6 part as sp_cyp_db_create wants it; chrom_seq = the bases of [window_start, window_start + window_len) */
int32_t sp_database_cyp_flatten(sp_database* db, const char* chrom_seq, uint64_t window_start, uint64_t window_len,
                                sp_cyp_locus* locus, sp_cyp_gene_def* gene_def, sp_cyp_config* config);

/* One variant-typed gene: load_database_haplotypes (src/diplotyper.rs:437-538) -- every defined haplotype normalised against the
 * chromosome (chrom_seq may be NULL: no reference, as NormalizedVariant::new without a genome), haplotypes with a variant that does
 * not normalise are dropped (n_skipped_haplotypes), the variant table is the BTreeMap<NormalizedVariant, VariantMeta> in key order --
 * and the gene's structural-variant definitions (PgxStructuralVariants + the database's gene_collection) for is_deletion. */
typedef struct sp_variant_gene sp_variant_gene;
int32_t sp_variant_gene_create(sp_database* db, const char* gene_name, const char* chrom_seq, uint64_t chrom_len, sp_variant_gene** out);
void    sp_variant_gene_free(sp_variant_gene* gene);
typedef struct { uint32_t n_haplotypes, n_variants, n_skipped_haplotypes, n_full_deletions, n_partial_deletions, reserved; } sp_variant_gene_stats;
int32_t sp_variant_gene_info(const sp_variant_gene* gene, sp_variant_gene_stats* out);
int32_t sp_variant_gene_haplotype(const sp_variant_gene* gene, uint32_t h, const char** name, const char** core_allele /* NULL: is one */);
int32_t sp_variant_gene_variant(const sp_variant_gene* gene, uint32_t v, uint64_t* position, const char** ref, const char** alt,
                                const char** name, const char** dbsnp_id /* may come back NULL */, int64_t* variant_id, int32_t* is_core);
int32_t sp_variant_gene_sv_definitions(const sp_variant_gene* gene, sp_sv_definitions* out);      /* for sp_variant_is_deletion */
int32_t sp_variant_gene_sv_label(const sp_variant_gene* gene, int32_t kind, int32_t index, const char** label);
/* load_vcf_variants + load_sv_vcf_variants (src/diplotyper.rs:551-857) after the file decoding: the caller hands over the decoded
 * records -- one sp_vcf_allele per ALT allele of a small-variant record (0-based position, REF, that ALT; gt = SP_GT_* of THIS allele
 * in the sample's GT, SP_GT_HOM_REF when the allele is not called; ps = phase set or -1), one sp_vcf_deletion per SVTYPE=DEL record
 * (0-based start, INFO/END).  The library normalises, matches the alleles to the gene's variants (+-50 bp window, the last matching
 * record wins), decides the deletions with is_deletion (gene span, max_sv_length; 0 = 1,000,000), and fills *problem for
 * sp_variant_solve.  Variant ids of the problem: the gene's variants and the observed deletions merged in NormalizedVariant order;
 * sp_variant_gene_problem_variant maps an id back (db_variant = index for sp_variant_gene_variant, or -1 and the deletion label).
 * Errors (SP_ERR_INVALID_ARG): a homozygous allele with a phase set, two records for the same deletion, a deleted gene without a
 * definition in the gene collection. */
typedef struct { uint64_t position; const char* ref; const char* alt; int32_t gt, reserved; int64_t ps; } sp_vcf_allele;
typedef struct { uint64_t start, end; int32_t gt, reserved; int64_t ps; } sp_vcf_deletion;
int32_t sp_variant_gene_problem(sp_variant_gene* gene, uint32_t n_alleles, const sp_vcf_allele* alleles, uint32_t n_deletions,
                                const sp_vcf_deletion* deletions, uint64_t max_sv_length, sp_variant_problem* problem);
int32_t sp_variant_gene_problem_variant(const sp_variant_gene* gene, int32_t id, int32_t* db_variant, const char** sv_label, uint64_t* sv_start,
                                        uint64_t* sv_end);
int32_t sp_variant_gene_problem_sv_label(const sp_variant_gene* gene, int32_t label_id, const char** label);   /* obs_sv_label ids */
const char* sp_variant_gene_last_error(const sp_variant_gene* gene);

/* The result file: StarphaseJson / PgxGeneDetails (src/data_types/starphase_json.rs:11-326) written as serde_json::to_writer_pretty
 * does (save_json, src/util/file_io.rs:37-52; two-space indent, struct fields in declaration order, gene_details in key order,
 * Option::None as null).  A sp_gene_details collects the parts; sp_result_insert applies one of the reference's constructors to it --
 * with that constructor's checks ("diplotypes and simple_diplotypes must be the same length", "diplotypes and inexact_diplotypes
 * must be the same length") and StarphaseJson::insert's ("Entry for <gene> is already occupied.") as SP_ERR_INVALID_ARG. */
typedef struct sp_result sp_result;
typedef struct sp_gene_details sp_gene_details;
int32_t sp_result_create(const sp_database* db /* NULL: PgxMetadata::default() */, const char* pbstarphase_version, sp_result** out);
void    sp_result_free(sp_result* result);
const char* sp_result_last_error(const sp_result* result);
int32_t sp_gene_details_create(sp_gene_details** out);
void    sp_gene_details_free(sp_gene_details* details);
int32_t sp_gene_details_add_diplotype(sp_gene_details* d, const char* hap1, const char* hap2);             /* Diplotype::new */
int32_t sp_gene_details_add_simple_diplotype(sp_gene_details* d, const char* hap1, const char* hap2);      /* simple_diplotypes: Some(..) */
int32_t sp_gene_details_set_simple_diplotypes(sp_gene_details* d, int32_t some);                           /* Some(vec![]) / None */
/* InexactDiplotype::new(InexactHaplotype::new(base, variants), ..): variants as for sp_inexact_haplotype */
int32_t sp_gene_details_add_inexact_diplotype(sp_gene_details* d,
                                              const char* base1, uint32_t n1, const char* const* labels1, const uint8_t* is_vi1, const int32_t* states1,
                                              const char* base2, uint32_t n2, const char* const* labels2, const uint8_t* is_vi2, const int32_t* states2);
int32_t sp_gene_details_add_diplotype_only(sp_gene_details* d, const char* hap1, const char* hap2);        /* InexactDiplotype::new_diplotype_only */
typedef struct {                                  /* PgxVariantDetails (:247-262); sv_label NULL = not a structural variant */
    uint64_t variant_id; const char* variant_name; const char* dbsnp;
    const char* chrom; uint64_t position; const char* reference; const char* alternate;
    const char* sv_label; uint64_t sv_start, sv_end;
    int32_t genotype /* SP_GT_* */, is_core_variant; int64_t phase_set /* -1 = None */;
} sp_variant_detail;
int32_t sp_gene_details_add_variant(sp_gene_details* d, const sp_variant_detail* v);
typedef struct { int32_t present, has_clips; uint64_t seq_len, nm, unmapped, clipped_start, clipped_end; } sp_mapping_stats;   /* Option<MappingStats> */
int32_t sp_gene_details_add_mapping(sp_gene_details* d, const char* read_qname, const char* best_hla_id, const char* best_star_allele,
                                    const sp_mapping_stats* cdna, const sp_mapping_stats* dna, int32_t is_ignored);       /* PgxMappingDetails */
int32_t sp_gene_details_add_multi_mapping(sp_gene_details* d, const char* read_qname, uint64_t read_start, uint64_t read_end,
                                          uint64_t consensus_id, const char* consensus_star_allele);                      /* PgxMultiMappingDetails */
enum { SP_DETAILS_SUBALLELE_MATCH = 0, SP_DETAILS_CORE_MATCH = 1, SP_DETAILS_INEXACT_DIPLOTYPES = 2, SP_DETAILS_FROM_MAPPINGS = 3,
       SP_DETAILS_FROM_MULTI_MAPPINGS = 4, SP_DETAILS_NO_MATCH = 5 };
int32_t sp_result_insert(sp_result* result, const char* gene, const sp_gene_details* details, int32_t constructor);
int32_t sp_result_json(sp_result* result, const char** text, uint64_t* len);
int32_t sp_result_save(sp_result* result, const char* path);                    /* gzip when the name ends in ".gz" */
/* save_pharmcat_tsv (src/main.rs:190-241): "#gene<TAB>diplotype" and one row per gene in key order -- the de-duplicated simple
 * diplotypes of the gene (PgxGeneDetails::dedup_simple_diplotypes: equal up to the order of the two haplotypes) give "Multiple/Multiple"
 * when more than one is left, else Diplotype::pharmcat_diplotype (a haplotype containing '+' in brackets); MT-RNR1 is written as its
 * single haplotype, "Unknown" when the two differ. */
int32_t sp_result_pharmcat_tsv(sp_result* result, const char** text, uint64_t* len);
int32_t sp_result_save_pharmcat_tsv(sp_result* result, const char* path);

/* ------------------------------------------------------------------ f4: the debug files (host only)
 * `hla_debug.json` (HlaDebug, src/hla/debug.rs:7-221; written by diplotype_hla_batch when a debug folder is given,
 * src/hla/caller.rs:1042-1048): per gene and read (or "consensus1" / "consensus2") the best match and the detailed mappings against the
 * alleles compared, and per gene the DualPassingStats of is_passing_dual (src/hla/caller.rs:1225-1247).  Errors as the reference's:
 * "Entry <x> is already occupied" (SP_ERR_INVALID_ARG, text from sp_hla_debug_last_error).
 * sp_aln_strings turns an alignment of this library (sp_align_batch with events; A = query, B = target) into what
 * DetailedMappingStats::from_mapping copies from minimap2 (:148-172): the CIGAR string (M / I / D, no --eqx), the MD tag and
 * match_len (matching bases); query_unmapped / target_unmapped are a_len - (a_end - a_start) and b_len - (b_end - b_start).
 * sp_affine_cigar_strings does the same for a mapping under the reference's scores (sp_affine_align_batch / sp_hla_realign_cigars): the dna_mapping of a
 * realigned read's ReadMappingStats (src/hla/caller.rs:575-577; the per-read records a host collects into a `read_debug.json`).
 * `cyp2d6_alleles.json` is written by sp_cyp_alleles_json above. */
typedef struct { int32_t present, reserved; uint64_t query_len, target_len, match_len, nm, query_unmapped, target_unmapped;
                 const char* cigar; const char* md; } sp_detailed_mapping;                    /* Option<DetailedMappingStats> */
int32_t sp_aln_strings(const sp_aln* aln, const uint32_t* events, const char* target, uint64_t target_len,
                       char* cigar, uint32_t cigar_cap, char* md, uint32_t md_cap, uint64_t* match_len);
/* the same strings for a mapping of sp_affine_align_batch / sp_hla_realign_cigars (a = query, b = target): '=' and 'X' merge into M, MD prints the target base
 * of every 'X' column and ^bases of a deletion, match_len is the number of '=' columns.  SP_ERR_INVALID_ARG when the ops do not consume exactly the spans of aln. */
int32_t sp_affine_cigar_strings(const sp_affine_aln* aln, const uint32_t* cigar, uint32_t n_cigar, const char* target, uint64_t target_len,
                                char* cigar_str, uint32_t cigar_cap, char* md, uint32_t md_cap, uint64_t* match_len);
/* the same with '=' and 'X' runs kept apart, as minimap2 writes a CIGAR under --eqx (score_read maps with flag 0x4000000, src/hla/caller.rs:1395: the cigar of
 * hla_debug.json's per-allele mappings); same arguments, same MD and match_len, same errors */
int32_t sp_affine_cigar_strings_eqx(const sp_affine_aln* aln, const uint32_t* cigar, uint32_t n_cigar, const char* target, uint64_t target_len,
                                char* cigar_str, uint32_t cigar_cap, char* md, uint32_t md_cap, uint64_t* match_len);
typedef struct sp_hla_debug sp_hla_debug;
int32_t sp_hla_debug_create(sp_hla_debug** out);
void    sp_hla_debug_free(sp_hla_debug* debug);
const char* sp_hla_debug_last_error(const sp_hla_debug* debug);
int32_t sp_hla_debug_add_read(sp_hla_debug* debug, const char* gene, const char* qname,
                              const char* best_match_id /* NULL: None */, const char* best_match_star);
int32_t sp_hla_debug_add_mapping(sp_hla_debug* debug, const char* gene, const char* qname, const char* hla_id,
                                 const sp_detailed_mapping* cdna, const sp_detailed_mapping* dna);
int32_t sp_hla_debug_add_dual_stats(sp_hla_debug* debug, const char* gene, const sp_hla_call* call);
int32_t sp_hla_debug_json(sp_hla_debug* debug, const char** text, uint64_t* len);
int32_t sp_hla_debug_save(sp_hla_debug* debug, const char* path);             /* gzip when the name ends in ".gz" */

/* ------------------------------------------------------------------ e: gathering the ranks' results (the path's one exchange step)
 * The reference has no counterpart: it is single-threaded and a cohort is N process runs (src/cli/diplotype.rs:185-191).  BASELINE.json's
 * north_star shards independent units (samples, genes) over the GPUs of a node, one process and one sp_ctx per GPU, with "RCCL over xGMI used
 * only to gather per-gene results" (SURVEY.md 8(b) sp_gather_results, 8(e)).  Rank 0 makes a 128-byte id (ncclGetUniqueId) and the host hands it
 * to the other ranks over whatever channel it has (a file, a socket, MPI, a torch store); every rank then joins the group on its context's device.
 * sp_gather_results: every rank contributes bytes_per_rank bytes of packed records (host memory) and receives all ranks' records in rank order
 * (n_ranks * bytes_per_rank bytes) -- one ncclAllGather on the context's stream, synchronous on return.  librccl is opened at run time; without it
 * sp_group_* fail with SP_ERR_NO_DEVICE and nothing else in the library is affected. */
typedef struct sp_group sp_group;
#define SP_GROUP_ID_BYTES 128
int32_t sp_group_unique_id(uint8_t* id /* SP_GROUP_ID_BYTES */);
int32_t sp_group_create(sp_ctx* ctx, const uint8_t* id, int32_t rank, int32_t n_ranks, sp_group** out);
void    sp_group_free(sp_group* group);
int32_t sp_group_size(const sp_group* group, int32_t* rank, int32_t* n_ranks);
int32_t sp_gather_results(sp_group* group, const void* records, uint64_t bytes_per_rank, void* all_records);

/* ------------------------------------------------------------------ f2: decoding the input files (host only)
 * What the reference gets from rust-htslib: the records of an indexed BAM that overlap a region (diplotype_hla_batch,
 * src/hla/caller.rs:523-596; the CYP2D6 read collection, src/cyp2d6/caller.rs:96-139) and the records of a VCF around a position
 * (load_vcf_variants / load_sv_vcf_variants, src/diplotyper.rs:551-857).  BGZF is read with zlib; a BAM is read through its .bai when
 * "<path>.bai" (or "<path minus .bam>.bai") exists and by a linear scan otherwise; a VCF (plain, gzip or bgzip) is read into memory
 * once -- no tabix index is needed for files of one sample's PGx-gene size, and none is used.  CRAM is not read.
 * Pointers handed out belong to the reader and stay valid until its next fetch call (or its free). */
typedef struct sp_bam sp_bam;
int32_t sp_bam_open(const char* path, sp_bam** out, char* err, uint32_t err_cap);
void    sp_bam_free(sp_bam* bam);
const char* sp_bam_last_error(const sp_bam* bam);
int32_t sp_bam_references(const sp_bam* bam, uint32_t* n, const char* const** names, const uint64_t** lengths);   /* @SQ of the header */
typedef struct {                                  /* one alignment record */
    const char* qname; uint32_t flag, mapq; int32_t ref_id, reserved; int64_t pos, end;   /* 0-based [pos, end) on the reference (end from the CIGAR) */
    uint32_t l_seq, n_cigar; const uint32_t* cigar;                                         /* BAM encoding: len << 4 | op */
} sp_bam_read;
/* the records overlapping [start, end) of chrom in file order; exclude_flags drops records with any of these FLAG bits; dedupe != 0
 * drops a record whose QNAME was handed out since sp_bam_open / sp_bam_forget (the reference's qnames_checked set, :532,565-570).
 * bases / offsets: the SEQ fields as stored (reference-forward ASCII, "=ACMGRSVTWYHKDBN"), concatenated, n + 1 offsets -- the
 * arguments of sp_seqset_upload. */
int32_t sp_bam_fetch(sp_bam* bam, const char* chrom, uint64_t start, uint64_t end, uint32_t exclude_flags, int32_t dedupe,
                     const sp_bam_read** reads, uint32_t* n, const char** bases, const uint64_t** offsets);
int32_t sp_bam_forget(sp_bam* bam);               /* empties the set of QNAMEs seen */
/* the SEQ fields of the records of the last fetch exactly as the file stores them (4 bits per base, high nibble first, every read on a
 * byte boundary): the arguments of sp_seqset_upload_format(ctx, SP_SEQ_BAM4, ...) -- half of what the ASCII form sends over PCIe */
int32_t sp_bam_last_seq4(const sp_bam* bam, const uint8_t** seq4, const uint64_t** byte_offsets, const uint32_t** lengths, uint32_t* n);

typedef struct sp_vcf sp_vcf;
int32_t sp_vcf_open(const char* path, sp_vcf** out, char* err, uint32_t err_cap);
void    sp_vcf_free(sp_vcf* vcf);
/* A BGZF-compressed VCF with a tabix (<path>.tbi) or CSI (<path>.csi) index beside it is opened by its header alone; every query below then reads only the chunks
 * the index names for its region (bcf::IndexedReader::fetch, src/diplotyper.rs:569-575,800) -- a 5 M-record WGS VCF costs a query a few blocks, not a scan.  Without
 * an index (or with one that cannot be read) the file is read once as a whole.  indexed: which of the two; lines_parsed_by_fetches: record lines the queries so far
 * have parsed (either may be NULL). */
int32_t sp_vcf_index_info(const sp_vcf* vcf, int32_t* indexed, uint64_t* lines_parsed_by_fetches);
const char* sp_vcf_last_error(const sp_vcf* vcf);
int32_t sp_vcf_samples(const sp_vcf* vcf, uint32_t* n, const char* const** names);
/* small variants: one sp_vcf_allele per ALT allele of every record of chrom that overlaps [start, end), for one sample (NULL = the
 * first); gt is the state of THAT allele in the sample's GT -- SP_GT_HOM_ALT a/a, SP_GT_HET_FLIP a|x, SP_GT_HET_PHASED x|a,
 * SP_GT_HET_UNPHASED a/x or x/a, SP_GT_HOM_REF when the allele is not called; ps = FORMAT/PS of a phased GT or -1.  Records whose GT
 * is missing or not diploid are skipped (src/diplotyper.rs:606-640).  The rows are the input of sp_variant_gene_problem. */
int32_t sp_vcf_alleles(sp_vcf* vcf, const char* sample, const char* chrom, uint64_t start, uint64_t end, const sp_vcf_allele** out, uint32_t* n);
/* structural variants (src/diplotyper.rs:739-857): single-ALT records of chrom with INFO/SVTYPE=DEL that overlap [start, end); the
 * deleted region is [POS - 1, INFO/END).  SP_ERR_INVALID_ARG where the reference bails: a record without SVTYPE or a DEL without END. */
int32_t sp_vcf_deletions(sp_vcf* vcf, const char* sample, const char* chrom, uint64_t start, uint64_t end, const sp_vcf_deletion** out, uint32_t* n);

/* ------------------------------------------------------------------ profiling hooks (bench.py)
 * HIP-event timing of the dominant kernel on the context's own stream. */
int32_t sp_profile_reset(sp_ctx* ctx);
int32_t sp_profile_get(sp_ctx* ctx, const char* kernel, double* total_ms, uint64_t* launches, uint64_t* cells);
/* device-side counters since the last sp_profile_reset come back in *cells under the names "count:k1_cells_active" (cells of the
 * first K1 pass whose gene the read anchors in), "count:k1_cells_executed" (those that ran the DP; the others were settled by prefix
 * sharing), "count:k1_cells_resumed" (executed cells that started from their predecessor's snapshot), "count:k1_cells_bytes"
 * (algorithmic bytes of the executed cells), "count:cons_launches", "count:cons_columns" (K8).
 * "pool:device": the context's pooled device buffers (its helpers' included) -- *launches = device allocations they have made since the context was created (never
 * reset; a call on a warm context adds none), *cells = bytes they hold.  Only the pooled buffers (sp_pool, the scratch) are counted: the buffers of a sequence set a
 * caller uploads or a database builds are that object's own and are not. */
/* roofline peaks measured on this device in this run: what = "valu_int" (v_add_u32 wave-instructions / s), "match16" (VALU
 * wave-instructions / s of the WFA cell's 16-base compare), "hbm_copy" (bytes / s, read + written, of a 2 x 1 GiB streaming copy) */
int32_t sp_microbench(sp_ctx* ctx, const char* what, double* rate);

/* The reference FASTA (ReferenceGenome::from_fasta / get_slice of rust-lib-reference-genome, loaded once in src/cli/diplotype.rs): the
 * slices sp_database_hla_gene / sp_database_cyp_window / sp_variant_gene_create ask for.  Plain files are read through "<path>.fai"
 * when it exists (only the requested bases are read), otherwise -- and for gzip / BGZF files -- the file is read into memory once.
 * Coordinates are 0-based half-open; bases come back upper-cased and stay valid until the next fetch on the handle. */
typedef struct sp_fasta sp_fasta;
int32_t sp_fasta_open(const char* path, sp_fasta** out, char* err, uint32_t err_cap);
void    sp_fasta_free(sp_fasta* fasta);
const char* sp_fasta_last_error(const sp_fasta* fasta);
int32_t sp_fasta_sequences(sp_fasta* fasta, uint32_t* n, const char* const** names, const uint64_t** lengths);
int32_t sp_fasta_fetch(sp_fasta* fasta, const char* chrom, uint64_t start, uint64_t end, const char** bases, uint64_t* len);

/* ------------------------------------------------------------------ files to files: the whole `diplotype` run
 * call_diplotypes (src/diplotyper.rs:40-330) behind one handle: the database, the reference FASTA and the per-database tables (HLA database,
 * CYP2D6 templates and typing tables, every variant gene normalised) are made once by sp_starphase_create; sp_starphase_call then types one sample
 * from its files -- variant genes from the VCF (+ SV VCF) in one sp_variant_solve_batch, the HLA genes of hla_config from the BAMs (K1 / K8 / K2,
 * PgxMappingDetails of every read), CYP2D6 from the BAMs (K3 / K8 / K9 / K7 / K4 / K5) -- and returns an sp_result for sp_result_save /
 * sp_result_save_pharmcat_tsv.  The CYP2D6 locus runs on a second context of the handle (same device), on a host thread of its own, beside the
 * variant genes and the HLA genes of the main context; `sequential` = 1 runs the three one after another on the calling thread.  The output does not
 * depend on which: every gene's entry is made from its own inputs alone.
 *
 * sp_diplotype_settings: DiplotypeSettings (src/cli/diplotype.rs:14-196) minus the inputs of one sample; sp_diplotype_settings_default fills the
 * reference's default_values (max_sv_length 1,000,000, max_error_rate 0.07, min_cdf_prob 0.001, expected_maf 0.45, min_consensus_fraction 0.10,
 * min_consensus_count 3, dual_max_ed_delta 100, every switch off, every path NULL).  include_set / exclude_set: files of gene names, one per line
 * (load_file_lines); sample_name NULL = the first sample of the VCF; sv_vcf: the SV VCF of every sample unless sp_sample_inputs names one.
 * debug_folder: hla_debug.json (per gene: the consensus matches and DualPassingStats) and cyp2d6_alleles.json are written there, and, after
 * sp_starphase_set_read_debug(handle, 1), read_debug.json (below); nothing else.
 * sp_diplotype_settings_check is check_diplotype_settings (:200-330) without the file-existence checks (a host does those; the command line exits
 * with NOINPUT): SP_ERR_INVALID_ARG with the reference's message in err ("Must provide a VCF file and/or aligned BAM file to perform diplotyping.",
 * "Only one of --exclude-set and --include-set can be specified.", "--max-error-rate must be between 0.0 and 1.0", ...); with BAMs and
 * disable_cdna_scoring it sets hla_require_dna as the reference does. */
typedef struct {
    const char* include_set; const char* exclude_set;   /* --include-set / --exclude-set (at most one) */
    const char* sample_name;                            /* --sample-name */
    const char* sv_vcf;                                 /* --sv-vcf */
    const char* debug_folder;                           /* --output-debug */
    uint64_t max_sv_length;                             /* --max-sv-length */
    int32_t  disable_cdna_scoring, hla_require_dna;     /* --disable-cdna-scoring, --hla-require-dna */
    double   max_error_rate, min_cdf_prob, expected_maf;/* --max-error-rate, --min-cdf-prob, --expected-maf */
    int32_t  infer_connections, normalize_d6_only;      /* --infer-connections, --normalize-d6-only */
    double   min_consensus_fraction;                    /* --min-consensus-fraction */
    uint64_t min_consensus_count, dual_max_ed_delta;    /* --min-consensus-count, --dual-max-ed-delta */
    int32_t  debug_skip_hla;                            /* --debug-skip-hla */
    int32_t  sequential;                                /* 1: variant genes, HLA, CYP2D6 one after another on the calling thread */
} sp_diplotype_settings;
typedef struct {
    uint32_t n_bams; const char* const* bams;           /* --bam, in the order given */
    const char* vcf;                                    /* --vcf or NULL */
    const char* sv_vcf;                                 /* NULL: settings.sv_vcf */
    const char* sample_name;                            /* NULL: settings.sample_name */
} sp_sample_inputs;
void    sp_diplotype_settings_default(sp_diplotype_settings* out);
int32_t sp_diplotype_settings_check(sp_diplotype_settings* settings, const sp_sample_inputs* inputs, char* err, uint32_t err_cap);
/* ctx: the context to run on, or NULL for one of the handle's own on device 0 (no device: SP_ERR_NO_DEVICE).  reference_fasta may be NULL (variant
 * genes are then normalised without a genome and a sample with BAMs fails: "Reference genome is required for reading alignment files").
 * The settings and their strings are copied.  A failed create returns no handle; sp_starphase_last_error(NULL) then gives the reason (per thread). */
typedef struct sp_starphase sp_starphase;
int32_t sp_starphase_create(sp_ctx* ctx, const char* database_path, const char* reference_fasta, const sp_diplotype_settings* settings, sp_starphase** out);
void    sp_starphase_free(sp_starphase* handle);
const char* sp_starphase_last_error(const sp_starphase* handle);
/* one sample: *out is a new sp_result (sp_result_free).  Errors as the reference's: a region fetch that fails counts as no reads (the warning is kept:
 * sp_starphase_warnings), an expected CYP2D6 CallerError gives the NO_MATCH entry, anything else fails the call (DATAERR on the command line).
 * On a caller's context in exhaustive K1 mode ("k1_best_n" = 0) no HLA read is named after a reverse-strand mapping (those come from the seeded stage). */
int32_t sp_starphase_call(sp_starphase* handle, const sp_sample_inputs* inputs, sp_result** out);
/* read_debug.json, off by default (enable 0): with the switch on, a call with a debug folder (settings.debug_folder; debug_folders[i] of sp_starphase_call_batch)
 * also writes <folder>/read_debug.json -- the reference's `read_debug` (src/hla/caller.rs:536,575-577,631-635): an HlaDebug object (sp_hla_debug_*) whose
 * read_mapping_stats hold, per gene and QNAME, best_match_id / best_match_star and mapping_stats = { <allele id>: { cdna_mapping: null, dna_mapping: { query_len,
 * target_len, match_len, nm, query_unmapped, target_unmapped, cigar, md } } }; dual_passing_stats is null.  Included are the reads with is_realigned() (a
 * RealignedHlaRecord exists: the records with status 0), in the bucket of the accepted allele's gene -- exactly the HLA mapping details of the result that are not
 * ignored.  A status-3 record (the segment did not map forward to the gene reference, src/hla/realigner.rs:332-342) has realigned_record None in the reference:
 * it keeps its PgxMappingDetails but gets no entry here, like status 1 and 2.  best_match_star is the star string of the read's mapping details ("HLA-A*01:01:01:01").
 * The mapping is the traceback of the record's own re-score (sp_hla_realign_cigars + sp_affine_cigar_strings): one extra pass over the accepted reads, several times
 * the cost of the K1 pass it explains.  With the switch off no kernel is launched and no memory is taken for it; every other output is the
 * same bytes either way. */
int32_t sp_starphase_set_read_debug(sp_starphase* handle, int32_t enable);
/* the per-allele mappings of hla_debug.json, off by default (on 0): with the switch on, a call with a debug folder fills read_mapping_stats[gene]["consensus1" |
 * "consensus2"].mapping_stats of <folder>/hla_debug.json with one PairedMappingStats per allowed allele of the gene (score_read maps with all_hla_targets = true,
 * src/hla/caller.rs:1398), keyed by the star allele joined with ':' (:1473-1476): cdna_mapping / dna_mapping are DetailedMappingStats::from_mapping
 * (src/hla/debug.rs:161-182) of the K2 map (sp_hla_map_type_consensus above) -- query_* the allele, target_* the gene-strand consensus, cigar with '=' / 'X'
 * (sp_affine_cigar_strings_eqx), md over the consensus bases; null where the level has no mapping, and cdna_mapping null with disable_cdna_scoring.  best_match_id /
 * best_match_star stay the call's typed allele.  A star allele that occurs twice among the allowed alleles is the reference's "Entry ... is already occupied!" error;
 * here the first entry stays and the later one is skipped with a line in sp_starphase_warnings / sp_starphase_sample_warnings.  The map runs once per group of a
 * batch, over every consensus of the group's samples that have a debug folder.  With the switch off nothing of this runs and every output is the same bytes; with
 * it on, every output but hla_debug.json is.  The switch can turn a call that succeeds into one that fails: the map is part of the HLA pass, so an error of
 * sp_hla_map_type_consensus (out of memory; an allele whose alignment has more than 4,096 runs, SP_ERR_CAPACITY) fails the pass -- in a batch the group then goes
 * through it once more sample by sample, as for every other failure of a shared pass, and only the samples whose own map fails are failed. */
int32_t sp_starphase_set_hla_debug_mappings(sp_starphase* handle, int32_t on);
/* hla_ties.json, off by default (on 0): with the switch on, a call with a debug folder also writes <folder>/hla_ties.json (sp_hla_ties_json above): keyed by gene in
 * name order, then "consensus1" / "consensus2" (the second for a dual call only, as in hla_debug.json), each the a = 5 scan's classes (sp_hla_map_ties, scan 1) of
 * sp_hla_map_type_consensus_ex on that consensus: typed_allele the call's, winner = best_mm2, names the full star names of the gene's allowed alleles.  Genes without a
 * call are omitted, as is a consensus that does not place; a sample whose BAMs hold no HLA read writes {}.  The map runs once per group of a batch, over every
 * consensus of the group's samples that have a debug folder -- the same ONE map call that serves sp_starphase_set_hla_debug_mappings when both are on.  Off: no launch,
 * no pooled memory, every output the same bytes.  On: every other output the same bytes; a sample's file in a batch is the file of its single call.  A failing map
 * fails the pass as described above. */
int32_t sp_starphase_set_hla_ties(sp_starphase* handle, int32_t on);
/* consensus_support.json, off by default (on 0): with the switch on, a call with a debug folder also writes <folder>/consensus_support.json (sp_consensus_support_json
 * above): keyed by gene in name order, then "consensus1" / "consensus2" (the second for a dual call only, as in hla_debug.json), each with the fields of
 * sp_support_summary, typed_allele (the star string of the call's typed allele, "HLA-A*01:01:01:01", or null) and the contested columns; genes without a call (no
 * realigned reads) are omitted: a sample whose BAMs hold no HLA read writes {}, a sample without BAMs has no HLA pass and gets none of its debug files.  The tables are sp_hla_consensus_support_cohort's over the reads, records, is_cons1 and
 * consensuses of the call itself; the full per-column table stays behind the API.  The pass runs once per group of a batch, over the samples of the group that
 * have a debug folder; each sample's file equals its single call's file.  With the switch off no kernel is launched, no pool memory is taken and every output is the
 * same bytes; with it on, every other output is still the same bytes.  A failure of the support pass fails the HLA pass, like the K2 map above: the switch can turn a
 * call that succeeds into one that fails (out of memory; an alignment of more than 4,096 runs, SP_ERR_CAPACITY) -- in a batch the group then goes through the pass
 * once more sample by sample, and only the samples whose own pass fails are failed.  CYP2D6 consensuses are not covered. */
int32_t sp_starphase_set_consensus_support(sp_starphase* handle, int32_t on);
/* cyp2d6_consensus_support.json, off by default (on 0) and a switch of its own (sp_starphase_set_consensus_support writes the HLA file only): with it on, a call with
 * a debug folder whose CYP2D6 call has status 0 also writes <folder>/cyp2d6_consensus_support.json (sp_cyp_support_json above) from sp_cyp_consensus_support_cohort over the
 * reads, the consensuses and the multi_mapping_details records of the call itself; a sample without CYP2D6 reads or without a call writes no file.  The CYP2D6 lane then
 * asks its calls for their consensuses (the calls are the same) and runs one support pass per group of a batch, over the samples of the group that have a debug
 * folder; each sample's file equals its single call's file.  Off: no launch, no pool memory, every output the same bytes; on: every other output the same bytes.  A
 * failure of the pass fails the sample's CYP2D6 entry (out of memory; an alignment of more than 4,096 runs, SP_ERR_CAPACITY); in a batch the group's samples then go
 * through the pass one by one and only those whose own pass fails are failed. */
int32_t sp_starphase_set_cyp_consensus_support(sp_starphase* handle, int32_t on);
/* cyp2d6_alleles.vcf.gz, off by default (on 0): with it on, a call with a debug folder whose CYP2D6 call has status 0 also writes <folder>/cyp2d6_alleles.vcf.gz
 * (sp_cyp_alleles_vcf_save above, FORMAT GT:SR:CR, flank SP_CYP_VCF_FLANK) from sp_cyp_variant_support_cohort over the samples of the batch group that have a debug
 * folder -- the SAME member pass that serves sp_starphase_set_cyp_consensus_support when both are on.  Off, or no debug folder: no launch, no file, and every output is
 * the same bytes; on: every other output is.  A failure of the pass or of the file fails the sample's CYP2D6 entry. */
int32_t sp_starphase_set_cyp_vcf(sp_starphase* handle, int32_t on);
/* cyp2d6_alternatives.json, off by default (on 0): with it on, the CYP2D6 lane's chain-pair search of a sample that has a debug folder is
 * sp_cyp_best_chain_pairs with max_alts 10 (the reference's heap size), whose entry 0 is the call, and a call of status 0 also writes
 * <folder>/cyp2d6_alternatives.json (sp_cyp_alternatives_json, without n_pairs_scored); a call that ends in an expected CallerError writes no file.  The single call,
 * a batch and the cohort call write the same bytes for a sample.  Off, or no debug folder: nothing more is launched or pooled and every output is the same bytes;
 * on: every other output is. */
int32_t sp_starphase_set_cyp_alternatives(sp_starphase* handle, int32_t on);
/* cyp2d6_alternative_reads.json, off by default (on 0): with it on, a sample that has a debug folder and a CYP2D6 call of status 0 also receives
 * <folder>/cyp2d6_alternative_reads.json (sp_cyp_alternative_reads_json): the observed-chain table and the SP_CYP_ALTERNATIVES best pairs read by read
 * (sp_cyp_chain_pair_reads on the pairs of the N-best search -- the ONE search that also serves cyp2d6_alternatives.json when both switches are on; either works
 * without the other), the reads named by their QNAMEs.  The single call, a batch and the cohort call write the same bytes for a sample.  Off, or no debug folder:
 * nothing more is launched or pooled and every output is the same bytes; on: every other output is. */
int32_t sp_starphase_set_cyp_alternative_reads(sp_starphase* handle, int32_t on);
/* variant_alternatives.json, off by default (on 0): with it on, the samples of a group that have a debug folder run one sp_variant_alternatives_batch
 * (n_best SP_VAR_ALTERNATIVES) beside the group's one sp_variant_solve_batch, and each receives <folder>/variant_alternatives.json: one object keyed by
 * gene name, in name order, with sp_variant_alternatives_json's entry for every variant gene solved for the sample (a gene answered without a solve --
 * no variants in the database -- has no entry).  The single call and a batch write the same bytes for a sample.  Off, or no debug folder: nothing more
 * is launched or pooled and every output is the same bytes; on: every other output is. */
int32_t sp_starphase_set_variant_alternatives(sp_starphase* handle, int32_t on);
/* A switch of its own, off by default, with effect only where one of the two switches above writes its file: the support pass of that file also makes the insertion
 * list (sp_hla_consensus_support_cohort_ins / sp_cyp_consensus_support_cohort_ins: the same one pass per batch group) and the file is rendered with it
 * (sp_consensus_support_json_ins / sp_cyp_support_json_ins, without first_read): every contested column with 2 * ins > depth gains "insertions" (and "more", "other").
 * Off: no further launch, no further pool memory, every output the same bytes as on a handle that was never told; on: every output but those two files the same bytes,
 * and a sample's file in a batch equals its single call's file. */
int32_t sp_starphase_set_support_insertions(sp_starphase* handle, int32_t on);
/* The same rule for the haplotype list: a switch of its own, off by default, with effect only where one of the two support switches writes its file.  The support pass
 * of that file also makes the list (sp_hla_consensus_support_cohort_hap / sp_cyp_consensus_support_cohort_hap: the same one pass per batch group, with the insertion
 * list only when that switch is on as well) and the file is rendered with it (sp_consensus_support_json_hap / sp_cyp_support_json_hap, without first_read): every
 * consensus or region whose list has columns and records gains "haplotypes".  Off: no further launch, no further pool memory, every output the same bytes as on a
 * handle that was never told; on: every output but those two files the same bytes, and a sample's file in a batch equals its single call's file. */
int32_t sp_starphase_set_support_haplotypes(sp_starphase* handle, int32_t on);
const char* sp_starphase_warnings(const sp_starphase* handle);      /* the warnings of the last call, one per line */
/* where the last call spent its time (wall ms): whole call, BAM decode (host, both loci), variant genes, HLA lane, CYP2D6 lane */
typedef struct { double call_ms, bam_decode_ms, variant_ms, hla_ms, cyp_ms; uint32_t n_hla_reads, n_cyp_reads; } sp_starphase_timing;
int32_t sp_starphase_last_timing(const sp_starphase* handle, sp_starphase_timing* out);
/* Many samples at once.  out[i] (sp_result_free) is what sp_starphase_call(handle, &inputs[i], ...) returns on the same handle: the same result
 * bytes, the same PharmCAT TSV and, when debug_folders[i] names a folder, the same hla_debug.json and cyp2d6_alleles.json as a single call with that
 * debug folder -- for every max_group and decode_threads, whichever samples share a group.  debug_folders: NULL, or n entries (NULL = none for that
 * sample); a handle created with settings.debug_folder needs them (else SP_ERR_INVALID_ARG: every sample would write the one folder).
 * Per group of max_group samples (default 64): the host decodes every sample's BAMs and VCFs on decode_threads workers (default min(16, hardware
 * threads)) -- while the device works on the group before --; the variant genes of all samples go through one sp_variant_solve_batch; the HLA reads
 * of all samples through one sp_hla_realign_reads_rev and one sp_hla_diplotype_cohort_samples; CYP2D6 through one sp_cyp_diplotype_cohort_mappings on
 * the handle's second context and a host thread of its own (settings.sequential: after the others).  Device memory is bounded by the group, not n.
 * A sample that fails gets out[i] = NULL, sample_rc[i] (optional) and its text in sp_starphase_sample_error(handle, i); the others are still typed
 * (a pass the group shares that fails as a whole is run again sample by sample, so each failure and its text are those of the sample's single call).
 * Returns the first status that is not SP_OK (sp_starphase_last_error names that sample).  Warnings are kept per sample. */
typedef struct {
    uint32_t max_group;                 /* samples per device pass; 0 = 64 */
    uint32_t decode_threads;            /* host BAM / VCF decode workers; 0 = min(16, hardware threads) */
    uint32_t reserved_[6];
} sp_batch_options;
int32_t sp_starphase_call_batch(sp_starphase* handle, uint32_t n, const sp_sample_inputs* inputs, const char* const* debug_folders /* optional */,
                                const sp_batch_options* opts /* NULL = defaults */, sp_result** out /* n */, int32_t* sample_rc /* n, optional */);
const char* sp_starphase_sample_error(const sp_starphase* handle, uint32_t i);      /* of the last batch; valid until the next call */
const char* sp_starphase_sample_warnings(const sp_starphase* handle, uint32_t i);
/* where the last batch spent its time (wall ms): the whole call; host decode (per group, the pool's wall time); variant genes, HLA lane, CYP2D6 lane
 * (its own thread, beside the two) and packaging summed over the groups; the counts */
typedef struct {
    double wall_ms, decode_ms, variant_ms, hla_ms, cyp_ms, package_ms;
    uint32_t n_samples, n_groups, n_failed, reserved_;
    uint64_t n_hla_reads, n_cyp_reads;
} sp_starphase_batch_timing;
int32_t sp_starphase_last_batch_timing(const sp_starphase* handle, sp_starphase_batch_timing* out);

/* ------------------------------------------------------------------ update-hla: a database's HLA section rebuilt from IMGT/HLA FASTA files
 * The HLA half of `pbstarphase build` without its downloads: the two files of an IMGT/HLA release a user keeps locally (hla_gen.fasta, hla_nuc.fasta) ->
 * the allele table (host) -> the gene coordinates stretched over every allele's best mapping (device) -> a database file `diplotype` can use (host).
 *
 * sp_hla_fasta_load: convert_fasta_str_to_map + collapse_hla_lookup (src/build_database.rs:233-325) + HlaAlleleDefinition::new (src/hla/alleles.rs:353-382).
 * The id is the record id, the star allele the first word of the description; a repeated id with the same (star allele, sequence) is accepted, with another it
 * fails with "FASTA record with multiple IDs/sequences detected: <id>"; a DNA record without a cDNA record is dropped (one warning with the count); a
 * description that differs between the files fails with `<id> has description "<dna>" for DNA and "<cdna>" for cDNA.`; an allele of a gene outside
 * SUPPORTED_HLA_GENES (alleles.rs:16-47) is dropped and counted; the table is in id order (the reference's BTreeMap).  Plain and gzip files are read.
 * Errors: SP_ERR_INVALID_ARG, no handle, the text in sp_hla_fasta_last_error() (per thread). */
typedef struct sp_hla_alleles sp_hla_alleles;
typedef struct {
    uint32_t n_alleles, n_dna;                        /* alleles kept; those of them with a DNA sequence */
    uint32_t n_dropped_no_cdna, n_dropped_gene;       /* DNA records without a cDNA record; alleles of unsupported genes */
    const char* warnings;                             /* one per line, "" when there are none */
} sp_hla_alleles_stats;
int32_t sp_hla_fasta_load(const char* hla_gen, const char* hla_nuc, sp_hla_alleles** out);
const char* sp_hla_fasta_last_error(void);
void    sp_hla_alleles_free(sp_hla_alleles* alleles);
int32_t sp_hla_alleles_info(const sp_hla_alleles* alleles, sp_hla_alleles_stats* out);
/* allele i in id order: "HLA:HLA00001", "HLA-A", "01:01:01:01", the DNA sequence (NULL: none) and the cDNA sequence; every output is optional */
int32_t sp_hla_alleles_get(const sp_hla_alleles* alleles, uint32_t i, const char** hla_id, const char** gene_name, const char** star_allele,
                           const char** dna, const char** cdna);

/* sp_hla_config_extend: HlaConfig::new (src/hla/alleles.rs:109-207).  The starting gene collection is the hla_config of `db` (the two-gene default when the file
 * has none, or db = NULL) reduced to SUPPORTED_HLA_GENES, with HLA-DRB3 / HLA-DRB4 copied from HLA-DRB1 when they are missing (HLA_COORDINATE_COPIES) and
 * HLA-DRB3 / 4 / 5 marked absent-capable (ABSENT_HLA_GENES).  Per gene, in name order: the window is [start - 2000, end + 2000) of the gene's INITIAL
 * coordinates on `reference`; every allele of the gene with a DNA sequence is mapped on it on both strands the library's way -- k-mer vote anchor
 * (sp_anchor_batch's kernel), then the two-piece affine re-score at the map-hifi scores on 256 diagonals around it (sp_affine_rescore_batch's kernel), which
 * reports minimap2's numbers; a cell whose score is below 200 is no mapping (map-hifi's min_dp_max: minimap2 drops it) -- back to back on the device, (allele, strand) cells of up to batch_alleles alleles (0 = 1,024; also bounded by bases, so memory
 * is bounded by the batch, not by the gene) per pass.  hlacfg_pick_extend_kernel then takes, per allele, its strands in minimap2's output order (higher DP
 * score first, forward first on a tie), keeps the one with the strictly smallest (nm + unmapped query bases) / allele length (0.1 for a zero numerator:
 * MappingScore::score_value) when that is strictly below 1.0, and folds window_start + t_start / t_end into the gene's minimum / maximum and the worst kept
 * score into the gene's slot (wave reduction, one partial per wave, a second small pass).  Comparisons are exact (integer cross-multiplication); ties for
 * "worst" go to the lowest allele index (the reference visits alleles in id order and replaces on strictly greater), so neither batch size nor launch
 * geometry changes a result.  extend_coordinates is src/database/gene_definition.rs:112-116: start = min, end = max, moved = either changed.
 * A window that starts before the chromosome (start < 2000; the reference's u64 subtraction underflows there and panics) or ends behind it fails the call
 * with SP_ERR_INVALID_ARG and a message.  An allele whose chosen re-score ends on the outermost diagonal of its band (the alignment may have left it) is
 * reported as "none" (status -1) with a warning naming it, as is one longer than 65,534 bases; neither fails the call (the reference skips an allele
 * without a mapping). */
typedef struct {
    int32_t status;                     /* 1 = mapping chosen; 0 = none (no DNA, no mapping, or no mapping scoring below 1.0); -1 = none: band overflow / too long */
    int32_t rev, nm;                    /* strand of the chosen mapping (1 = reverse), minimap2's NM */
    int32_t q_start, q_end;             /* span on the allele as given (minimap2 reports query coordinates on the query's own strand) */
    int32_t t_start, t_end;             /* span on the window: chromosome position = gene start - 2000 + t */
    int32_t gene;                       /* index into the result's genes, -1: the allele's gene is not in the collection */
} sp_hla_cfg_mapping;
typedef struct {
    const char* name; const char* chrom;
    uint64_t start, end;                /* the extended coordinates, 0-based half-open */
    int32_t  moved, is_absent_capable;
    int32_t  worst_allele;              /* index (sp_hla_alleles order) of the worst accepted mapping, -1: none beat the perfect match of the window */
    int32_t  worst_len, worst_nm, worst_unmapped;     /* its MappingStats */
    uint32_t n_dna_alleles, n_mapped;
} sp_hla_cfg_gene;
typedef struct sp_hla_config_result sp_hla_config_result;
int32_t sp_hla_config_extend(sp_ctx* ctx, sp_fasta* reference, const sp_database* db, const sp_hla_alleles* alleles, uint32_t batch_alleles,
                             sp_hla_config_result** out);
/* a result made by hand (host only): genes by name with their coordinates; moved = 0, no mappings */
int32_t sp_hla_config_result_create(uint32_t n_genes, const char* const* names, const uint64_t* start, const uint64_t* end, sp_hla_config_result** out);
void    sp_hla_config_result_free(sp_hla_config_result* result);
int32_t sp_hla_config_result_info(const sp_hla_config_result* result, uint32_t* n_genes, uint32_t* n_alleles, const char** warnings);
int32_t sp_hla_config_result_gene(const sp_hla_config_result* result, uint32_t g, sp_hla_cfg_gene* out);           /* g < n_genes, name order */
int32_t sp_hla_config_result_mapping(const sp_hla_config_result* result, uint32_t allele, sp_hla_cfg_mapping* out); /* allele < n_alleles */

/* The input database written again with its HLA part replaced (host only): hla_sequences = the table (HlaAlleleDefinition's fields in its order,
 * src/hla/alleles.rs:332-344), hla_config = { gene_collection: { version, gene_dict } } with the result's genes (GeneDefinition's fields in its order,
 * src/database/gene_definition.rs:18-34; a gene's transcript id, strand and exons are the input's, or the default's), database_metadata.hla_version =
 * hla_version; members in PgxDatabase's order (src/database/pgx_database.rs:23-41); every other section is carried over with unchanged content.  gzip when
 * out_path ends in ".gz".  A result gene the input's hla_config cannot supply (neither itself nor its HLA_COORDINATE_COPIES source), or one without an exon
 * (validate_config), fails with SP_ERR_INVALID_ARG (sp_database_last_error). */
int32_t sp_database_save_hla(const sp_database* db, const sp_hla_alleles* alleles, const sp_hla_config_result* result, const char* hla_version,
                             const char* out_path);

#ifdef __cplusplus
}
#endif
#endif

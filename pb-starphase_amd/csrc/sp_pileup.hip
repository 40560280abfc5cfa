// sp_pileup.hip -- many alignments -> integer counts per target column (sp_pileup_batch), the insertion and haplotype lists behind the table, and sp_align_pileup_batch:
// alignment, pileup, summary and lists in one device-resident pass.  The consensus support of HLA and CYP2D6 calls (sp_support.hip) runs on that pass.  Contract:
// include/starphase_hip.h; design: DESIGN.md section 7.2.
#include "sp_internal.h"
#include "sp_json.h"
#include <algorithm>
#include <atomic>
#include <cstring>
#include <numeric>

namespace {

// one alignment as pileup_kernel reads it, in bucket (target) order
struct PuPair { uint64_t op_off; uint32_t a, n_ops; int32_t b_start, a_start; };      // 24 bytes
struct PuTile { uint32_t target, c0; };

constexpr int PU_TILE = SP_PILEUP_TILE, PU_WAVES = SP_PILEUP_WAVES;
// The tile's counters live in LDS as one plane per field of sp_pileup_col, PU_STRIDE words apart: the lanes of a run add to consecutive words of one plane (one bank
// each), and the 32 lanes of a half wave that writes the tile out (8 fields x 4 columns of the array-of-structs output) read bank 4 f + column: no two alike.
// (Worked out from the bank rule -- 32 banks of 4 bytes for 4-byte LDS accesses -- not measured with the bank-conflict counter.)
constexpr int PU_STRIDE = PU_TILE + 4;
constexpr size_t PU_LDS_BYTES = (size_t)8 * PU_STRIDE * sizeof(uint32_t);              // 65,664 bytes: two workgroups per CU (160 KiB)
constexpr int PU_SHORT = 8;                                                            // runs of up to this many columns are expanded by their own lane, longer ones by the wave
enum { PU_DEPTH = 0, PU_EQ = 1, PU_X = 2, PU_DEL = 6, PU_INS = 7 };                    // plane = word of sp_pileup_col

__device__ __forceinline__ uint32_t pu_query_code(const uint32_t* words, int q) { return (words[q >> 4] >> ((q & 15) << 1)) & 3u; }

// one column of one run: op 7 '=', 8 'X', 2 'D'
__device__ __forceinline__ void pu_add(uint32_t* lds, int col, uint32_t op, const uint32_t* qwords, int q) {
    atomicAdd(&lds[PU_DEPTH * PU_STRIDE + col], 1u);
    const int plane = op == 7u ? PU_EQ : op == 2u ? PU_DEL : PU_X + (int)pu_query_code(qwords, q);
    atomicAdd(&lds[plane * PU_STRIDE + col], 1u);
}

// The walk over an op row (row / n_ops / b_start / a_start wave-uniform): the wave takes the ops 64 at a time, two wave-wide inclusive prefix sums give every op its first
// target column t0 and query base q0, and f(live, op, len, t0, q0) is called once per chunk on ALL 64 lanes (the callers ballot and shuffle inside).  A chunk that
// begins behind column `stop` (wave-uniform) ends the walk.
template <class F> __device__ __forceinline__ void pu_walk(const uint32_t* __restrict__ row, uint32_t n_ops, int b_start, int a_start, int lane, int stop, F f) {
    int tpos = b_start, qpos = a_start;                                                // first target column / query base of the chunk (wave-uniform)
    for (uint32_t k0 = 0; k0 < n_ops && tpos <= stop; k0 += SP_WAVE) {
        const bool live = k0 + lane < n_ops;
        const uint32_t w = live ? row[k0 + lane] : 0u;
        const uint32_t op = w & 15u; const int n = (int)(w >> 4);
        const int tl = (op == 7u || op == 8u || op == 2u) ? n : 0, ql = (op == 7u || op == 8u || op == 1u) ? n : 0;
        int ts = tl, qs = ql;                                                          // inclusive prefix sums over the chunk
#pragma unroll
        for (int d = 1; d < SP_WAVE; d <<= 1) {
            const int u = __shfl_up(ts, d), v = __shfl_up(qs, d);
            if (lane >= d) { ts += u; qs += v; }
        }
        const int t0 = tpos + ts - tl, q0 = qpos + qs - ql;                            // this op's first target column and query base
        tpos += __shfl(ts, SP_WAVE - 1); qpos += __shfl(qs, SP_WAVE - 1);
        f(live, op, n, t0, q0);
    }
}

// One alignment under one tile: the columns of its ops inside [c0, c1) are added to the tile's planes.  The walk is pu_walk's, written out: through pu_walk
// pileup_kernel kept its registers, yet ran 0.622-0.626 ms where the parent's spread was 0.593-0.598 ms (2,108 pairs; profiles/support/refactor.txt, section 1, state B).
__device__ __forceinline__ void pu_pair(uint32_t* lds, int c0, int c1, const uint32_t* qwords, const uint32_t* __restrict__ row, uint32_t n_ops, int b_start, int a_start, int lane) {
    int tpos = b_start, qpos = a_start;                                                // first target column / query base of the chunk (wave-uniform)
    for (uint32_t k0 = 0; k0 < n_ops && tpos <= c1; k0 += SP_WAVE) {                   // (an 'I' op at column c1 counts for column c1 - 1: <=)
        const bool live = k0 + lane < n_ops;
        const uint32_t w = live ? row[k0 + lane] : 0u;
        const uint32_t op = w & 15u; const int n = (int)(w >> 4);
        const int tl = (op == 7u || op == 8u || op == 2u) ? n : 0, ql = (op == 7u || op == 8u || op == 1u) ? n : 0;
        int ts = tl, qs = ql;                                                          // inclusive prefix sums over the chunk
#pragma unroll
        for (int d = 1; d < SP_WAVE; d <<= 1) {
            const int u = __shfl_up(ts, d), v = __shfl_up(qs, d);
            if (lane >= d) { ts += u; qs += v; }
        }
        const int t0 = tpos + ts - tl, q0 = qpos + qs - ql;                            // this op's first target column and query base
        tpos += __shfl(ts, SP_WAVE - 1); qpos += __shfl(qs, SP_WAVE - 1);
        if (live && op == 1u && t0 - 1 >= c0 && t0 - 1 < c1) atomicAdd(&lds[PU_INS * PU_STRIDE + (t0 - 1 - c0)], 1u);
        const int lo = max(t0, c0), hi = min(t0 + tl, c1);                             // the op's columns inside the tile
        const bool hit = live && tl > 0 && lo < hi;
        if (hit && tl <= PU_SHORT) for (int c = lo; c < hi; ++c) pu_add(lds, c - c0, op, qwords, q0 + (c - t0));
        unsigned long long longs = __ballot(hit && tl > PU_SHORT);
        while (longs) {                                                                // long runs: the wave's lanes across the run's columns
            const int src = __ffsll((long long)longs) - 1; longs &= longs - 1;
            const int rlo = __shfl(lo, src), rhi = __shfl(hi, src), rt0 = __shfl(t0, src), rq0 = __shfl(q0, src);
            const uint32_t rop = (uint32_t)__shfl((int)op, src);
            for (int c = rlo + lane; c < rhi; c += SP_WAVE) pu_add(lds, c - c0, rop, qwords, rq0 + (c - rt0));
        }
    }
}

__global__ __launch_bounds__(PU_WAVES * SP_WAVE) void pileup_kernel(SeqSetView A, const int32_t* __restrict__ t_len, const PuPair* __restrict__ pairs, const uint32_t* __restrict__ bucket_off,
                                                                    const uint32_t* __restrict__ ops, const PuTile* __restrict__ tiles, const uint64_t* __restrict__ col_offset,
                                                                    uint32_t* __restrict__ out) {
    extern __shared__ uint32_t lds[];
    const PuTile tile = tiles[blockIdx.x];
    const int c0 = (int)tile.c0, c1 = min(c0 + PU_TILE, t_len[tile.target]);           // the tile's columns [c0, c1)
    for (int i = threadIdx.x; i < 8 * PU_STRIDE; i += PU_WAVES * SP_WAVE) lds[i] = 0u;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (uint32_t p = bucket_off[tile.target] + wave; p < bucket_off[tile.target + 1]; p += PU_WAVES) {
        const PuPair pr = pairs[p];
        pu_pair(lds, c0, c1, A.words + A.word_off[pr.a], ops + pr.op_off, pr.n_ops, pr.b_start, pr.a_start, lane);
    }
    __syncthreads();
    uint32_t* dst = out + (col_offset[tile.target] + (uint64_t)c0) * 8u;                // the tile as an array of sp_pileup_col: consecutive threads, consecutive words
    for (int i = threadIdx.x; i < (c1 - c0) * 8; i += PU_WAVES * SP_WAVE) dst[i] = lds[(i & 7) * PU_STRIDE + (i >> 3)];
}

// ------------------------------------------------------------------------------------------------------------------------------
// sp_align_pileup_batch: the same tile, fed from what the map kernel (sp_launch_affine_map) left in device memory.  `order` lists the batch's pairs by target and, inside
// a target, in the order given, so the pairs of target t that fall into slice s of the batch are order[boff[t * (n_slices + 1) + s] .. boff[t * (n_slices + 1) + s + 1]).
// Slice 0 starts every tile from zero; a later slice loads the tile as the slices before it left it, adds its own pairs and stores it again -- the workgroup is the
// tile's one owner in its launch, the launches follow one another on one stream: plain loads and stores.  A tile none of the slice's pairs names is left as it is.
// The load is the store's transposition: 32 lanes write bank 4 f + column of the planes (PU_STRIDE = 4 mod 32), no two alike (derived from the bank rule, as above).
// ------------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t AP_LOST = 0xFFFFFFFFu;                   // n_cigar of a walk that did not arrive, op_off of a row that was not kept (sp_launch_affine_map)
constexpr uint64_t AP_NO_OPS = ~0ull;

// the pairs the table counts (wave-uniform): a row of ops that was kept (the host reports the other two) and an alignment.  Host op rows are staged with score 1.
__device__ __forceinline__ bool ap_counted(uint32_t n_ops, uint64_t off, const sp_affine_aln* g) { return n_ops != 0 && n_ops != AP_LOST && off != AP_NO_OPS && g->score > 0; }

// A wave takes its places in a list with one ballot and one atomic on the list's counter: the place of a lane that wants one (all 64 lanes call).
template <class T> __device__ __forceinline__ T wave_append(bool want, T* count, int lane) {
    const unsigned long long vote = __ballot(want);
    if (!vote) return 0;
    const int leader = __ffsll((long long)vote) - 1;
    T base = 0;
    if (lane == leader) base = atomicAdd(count, (T)__popcll(vote));
    return __shfl(base, leader) + (T)__popcll(vote & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(PU_WAVES * SP_WAVE) void pileup_rows_kernel(SeqSetView A, const int32_t* __restrict__ t_len, const sp_pair* __restrict__ pairs, const sp_affine_aln* __restrict__ aln,
                                                                         const uint32_t* __restrict__ n_cigar, const uint64_t* __restrict__ op_off, const uint32_t* __restrict__ ops,
                                                                         const uint32_t* __restrict__ order, const uint32_t* __restrict__ boff, uint32_t n_slices, uint32_t slice,
                                                                         const PuTile* __restrict__ tiles, const uint64_t* __restrict__ col_offset, uint32_t* __restrict__ out) {
    extern __shared__ uint32_t lds[];
    const PuTile tile = tiles[blockIdx.x];
    const uint32_t k_lo = boff[(size_t)tile.target * (n_slices + 1) + slice], k_hi = boff[(size_t)tile.target * (n_slices + 1) + slice + 1];
    if (slice > 0 && k_lo == k_hi) return;                                              // (uniform over the workgroup)
    const int c0 = (int)tile.c0, c1 = min(c0 + PU_TILE, t_len[tile.target]);
    uint32_t* dst = out + (col_offset[tile.target] + (uint64_t)c0) * 8u;
    if (slice == 0) for (int i = threadIdx.x; i < 8 * PU_STRIDE; i += PU_WAVES * SP_WAVE) lds[i] = 0u;
    else for (int i = threadIdx.x; i < (c1 - c0) * 8; i += PU_WAVES * SP_WAVE) lds[(i & 7) * PU_STRIDE + (i >> 3)] = dst[i];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (uint32_t k = k_lo + wave; k < k_hi; k += PU_WAVES) {
        const uint32_t p = order[k], n_ops = n_cigar[p];
        const uint64_t off = op_off[p];
        if (!ap_counted(n_ops, off, aln + p)) continue;
        const sp_affine_aln g = aln[p];
        pu_pair(lds, c0, c1, A.words + A.word_off[pairs[p].a], ops + off, n_ops, g.b_start, g.a_start, lane);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (c1 - c0) * 8; i += PU_WAVES * SP_WAVE) dst[i] = lds[(i & 7) * PU_STRIDE + (i >> 3)];
}

// ------------------------------------------------------------------------------------------------------------------------------
// Window support (sp_window_support; contract: include/starphase_hip.h, design: DESIGN.md section 7.2).  One workgroup per (target, chunk of WIN_CHUNK windows); lane l of
// every wave keeps windows l, l + 64, ... of the chunk and their counters in registers, the waves take the target's pairs of the slice in turn (order / boff as
// pileup_rows_kernel reads them).  A pair is walked once, and only when it spans one of the wave's windows: the defects of its op row go into the wave's part of LDS in
// doubled coordinates -- column c is [2 c, 2 c + 1), the junction behind column j is [2 j + 1, 2 j + 2), so window [s, e) is [2 s, 2 e - 1): its columns and its INTERIOR
// junctions --, sorted and disjoint by construction (ops follow one another on the target, an 'I' lies between two of them).  A window is inexact when the first defect
// that ends behind its start begins in front of its end.  A row with more defects than the wave's part holds is decided in rounds.  The waves' counters meet in LDS,
// thread i stores window i (slice > 0: on top of what the slices before it left).  No atomics.
// ------------------------------------------------------------------------------------------------------------------------------
struct WinChunk { uint32_t target, w0; };
constexpr int WIN_CHUNK = SP_WINDOW_CHUNK, WIN_WAVES = SP_WINDOW_WAVES, WIN_DEFECTS = SP_WINDOW_DEFECTS, WIN_PER_LANE = WIN_CHUNK / SP_WAVE;
static_assert(WIN_CHUNK % SP_WAVE == 0 && WIN_PER_LANE <= 32 && WIN_DEFECTS >= 2 * SP_WAVE && WIN_CHUNK <= WIN_WAVES * SP_WAVE, "a lane's windows are bits of one word; a round takes 64 ops; one thread stores one window");

// what one wave wrote to LDS is read by its other lanes: the compiler must not move the accesses across, the hardware keeps a wave's LDS accesses in order
__device__ __forceinline__ void win_wave_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }

__global__ __launch_bounds__(WIN_WAVES * SP_WAVE) void window_kernel(const sp_affine_aln* __restrict__ aln, const uint32_t* __restrict__ n_cigar, const uint64_t* __restrict__ op_off,
                                                                     const uint32_t* __restrict__ ops, const uint32_t* __restrict__ order, const uint32_t* __restrict__ boff,
                                                                     uint32_t n_slices, uint32_t slice, const WinChunk* __restrict__ chunks, const uint32_t* __restrict__ win_off,
                                                                     const sp_window* __restrict__ windows, sp_window_support* __restrict__ out) {
    __shared__ int2 s_def[WIN_WAVES][WIN_DEFECTS];
    __shared__ uint32_t s_cnt[WIN_WAVES][3][WIN_CHUNK];
    const WinChunk ch = chunks[blockIdx.x];
    const uint32_t k_lo = boff[(size_t)ch.target * (n_slices + 1) + slice], k_hi = boff[(size_t)ch.target * (n_slices + 1) + slice + 1];
    if (slice > 0 && k_lo == k_hi) return;                                              // (uniform over the workgroup)
    const uint32_t w_base = win_off[ch.target] + ch.w0, n_w = min((uint32_t)WIN_CHUNK, win_off[ch.target + 1] - w_base);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int w_lo[WIN_PER_LANE], w_hi[WIN_PER_LANE];                                         // a lane's windows (a place behind n_w: the empty window, which nothing counts)
    uint32_t c_span[WIN_PER_LANE], c_exact[WIN_PER_LANE], c_part[WIN_PER_LANE];
    int cmin = 0x7FFFFFFF, cmax = 0;                                                    // the columns the chunk's windows lie in: [cmin, cmax)
#pragma unroll
    for (int j = 0; j < WIN_PER_LANE; ++j) {
        const uint32_t i = (uint32_t)(lane + j * SP_WAVE);
        w_lo[j] = 0; w_hi[j] = 0; c_span[j] = 0; c_exact[j] = 0; c_part[j] = 0;
        if (i < n_w) { const sp_window w = windows[w_base + i]; w_lo[j] = (int)w.start; w_hi[j] = (int)w.end; cmin = min(cmin, w_lo[j]); cmax = max(cmax, w_hi[j]); }
    }
#pragma unroll
    for (int d = 1; d < SP_WAVE; d <<= 1) { cmin = min(cmin, __shfl_xor(cmin, d)); cmax = max(cmax, __shfl_xor(cmax, d)); }
    int2* def = s_def[wave];
    for (uint32_t k = k_lo + wave; k < k_hi; k += WIN_WAVES) {
        const uint32_t p = order[k], n_ops = n_cigar[p];
        const uint64_t off = op_off[p];
        if (!ap_counted(n_ops, off, aln + p)) continue;                                 // (everything up to the walk is wave-uniform)
        const sp_affine_aln g = aln[p];
        if (g.b_end <= cmin || g.b_start >= cmax) continue;                             // the pair meets none of the chunk's windows
        uint32_t spans = 0, bad = 0;                                                    // bit j: the pair spans the lane's window j / a defect lies in it
#pragma unroll
        for (int j = 0; j < WIN_PER_LANE; ++j) if (w_lo[j] < w_hi[j] && g.b_start <= w_lo[j] && w_hi[j] <= g.b_end) spans |= 1u << j;
        if (__ballot(spans != 0u)) {
            int n_def = 0;                                                              // defects in the wave's part (wave-uniform)
            auto decide = [&]() {                                                       // the lane's spanned windows against the defects held
                win_wave_sync();
#pragma unroll
                for (int j = 0; j < WIN_PER_LANE; ++j) {
                    if (!((spans & ~bad) >> j & 1u)) continue;
                    const int L = 2 * w_lo[j], H = 2 * w_hi[j] - 1;
                    int lo = 0, hi = n_def;
                    while (lo < hi) { const int mid = (lo + hi) >> 1; if (def[mid].y <= L) lo = mid + 1; else hi = mid; }
                    if (lo < n_def && def[lo].x < H) bad |= 1u << j;
                }
                win_wave_sync();
            };
            pu_walk(ops + off, n_ops, g.b_start, g.a_start, lane, cmax, [&](bool live, uint32_t op, int len, int t0, int) {
                if (n_def + SP_WAVE > WIN_DEFECTS) { decide(); n_def = 0; }
                const bool is_def = live && (op == 8u || op == 2u || op == 1u);
                const unsigned long long vote = __ballot(is_def);
                if (is_def) def[n_def + __popcll(vote & ((1ull << lane) - 1ull))] = op == 1u ? make_int2(2 * t0 - 1, 2 * t0) : make_int2(2 * t0, 2 * (t0 + len) - 1);
                n_def += __popcll(vote);
            });
            decide();
        }
#pragma unroll
        for (int j = 0; j < WIN_PER_LANE; ++j) {
            const bool sp = (spans >> j & 1u) != 0u, meets = w_lo[j] < w_hi[j] && g.b_start < w_hi[j] && w_lo[j] < g.b_end;
            c_span[j] += sp ? 1u : 0u; c_exact[j] += (sp && !(bad >> j & 1u)) ? 1u : 0u; c_part[j] += (meets && !sp) ? 1u : 0u;
        }
    }
#pragma unroll
    for (int j = 0; j < WIN_PER_LANE; ++j) { s_cnt[wave][0][lane + j * SP_WAVE] = c_span[j]; s_cnt[wave][1][lane + j * SP_WAVE] = c_exact[j]; s_cnt[wave][2][lane + j * SP_WAVE] = c_part[j]; }
    __syncthreads();
    if (threadIdx.x < n_w) {
        sp_window_support r = { 0, 0, 0, 0 };
        if (slice > 0) r = out[w_base + threadIdx.x];
        for (int w = 0; w < WIN_WAVES; ++w) { r.span += s_cnt[w][0][threadIdx.x]; r.exact += s_cnt[w][1][threadIdx.x]; r.partial += s_cnt[w][2][threadIdx.x]; }
        r.reserved_ = 0;
        out[w_base + threadIdx.x] = r;
    }
}

// what the host has to know about a slice before it piles it up: status[0] = a walk got lost, status[1] = an alignment with more runs than a row keeps
__global__ void ap_status_kernel(const sp_affine_aln* __restrict__ aln, const uint32_t* __restrict__ n_cigar, const uint64_t* __restrict__ op_off, uint32_t n, uint32_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (n_cigar[i] == AP_LOST) status[0] = 1u;
    else if (aln[i].score > 0 && op_off[i] == AP_NO_OPS) status[1] = 1u;
}

// The second try of a slice (retry_band of sp_align_pileup_band_batch), decided on the device.  One thread per pair of the slice: a pair that was attempted (max_ed >= 0)
// and came back from the first map launch with score 0 or without ops goes onto the retry list.  A wave takes its places with one ballot and one atomic on the list's
// counter; tried[i] (optional) keeps the decision for band_used.
__global__ void ap_retry_list_kernel(const sp_pair* __restrict__ pairs, const sp_affine_aln* __restrict__ aln, const uint32_t* __restrict__ n_cigar, uint32_t n,
                                     uint32_t* __restrict__ list, uint32_t* __restrict__ count, uint32_t* __restrict__ tried) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & (SP_WAVE - 1);
    const bool want = i < n && pairs[i].max_ed >= 0 && (aln[i].score <= 0 || n_cigar[i] == 0);
    const uint32_t at = wave_append(want, count, lane);
    if (want) list[at] = i;
    if (i < n && tried) tried[i] = want ? 1u : 0u;
}

// The list in pair order (the waves took their places in the order they arrived): entry k goes to the place of its rank among the *count distinct pair numbers.  The
// second launch then meets the pairs, and takes its op rows, in an order that depends on the results of the first alone.
__global__ void ap_retry_sort_kernel(const uint32_t* __restrict__ list, const uint32_t* __restrict__ count, uint32_t* __restrict__ sorted) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x, n = *count;
    if (k >= n) return;
    const uint32_t v = list[k];
    uint32_t rank = 0;
    for (uint32_t x = 0; x < n; ++x) rank += list[x] < v ? 1u : 0u;
    sorted[rank] = v;
}

// band_used: 0 for a pair without an alignment, else the band its alignment came from (in place over tried[]: the second try's when the pair was on the retry list)
__global__ void ap_band_used_kernel(const sp_affine_aln* __restrict__ aln, const uint32_t* __restrict__ n_cigar, uint32_t n, uint32_t band, uint32_t retry_band, int has_tried,
                                    uint32_t* __restrict__ tried_then_band) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool second = has_tried && tried_then_band[i] != 0u;
    tried_then_band[i] = (aln[i].score > 0 && n_cigar[i] > 0) ? (second ? retry_band : band) : 0u;
}

// sp_support_summarize per target, on the device.  One workgroup per target, one pass over its columns: the minimum depth and the contested columns fall out of it, and a
// histogram of the depths in LDS gives the lower median -- element (length - 1) / 2 of the sorted depths is the first bin at which the running count exceeds that rank.
// A depth is at most the number of pairs that name the target.  With more possible depths than AP_BINS the bins are W = ceil(range / AP_BINS) depths wide, and the bin the
// median falls into is resolved by another pass over the columns on that bin's W depths alone (rank reduced by the count below the bin), until W is 1.  Integers only.
constexpr int AP_SUM_THREADS = 256, AP_BINS = SP_SUPPORT_HIST_BINS;
static_assert(AP_BINS % AP_SUM_THREADS == 0, "bins per thread");

__global__ __launch_bounds__(AP_SUM_THREADS) void support_summary_kernel(const uint32_t* __restrict__ table, const uint64_t* __restrict__ col_offset, const int32_t* __restrict__ t_len,
                                                                          const sp_affine_aln* __restrict__ aln, const uint32_t* __restrict__ order, const uint32_t* __restrict__ boff,
                                                                          uint32_t n_slices, const uint32_t* __restrict__ n_members, sp_support_summary* __restrict__ out) {
    __shared__ uint32_t hist[AP_BINS], part[AP_SUM_THREADS], s_min, s_cont, s_al, s_lo, s_k;
    const uint32_t t = blockIdx.x, tid = threadIdx.x;
    const uint32_t len = (uint32_t)t_len[t], k_lo = boff[(size_t)t * (n_slices + 1)], k_hi = boff[(size_t)t * (n_slices + 1) + n_slices];
    if (tid == 0) { s_min = 0xFFFFFFFFu; s_cont = 0; s_al = 0; }
    __syncthreads();
    {
        uint32_t al = 0;
        for (uint32_t k = k_lo + tid; k < k_hi; k += AP_SUM_THREADS) al += aln[order[k]].score > 0 ? 1u : 0u;
        if (al) atomicAdd(&s_al, al);
    }
    const uint4* cols = (const uint4*)(table + col_offset[t] * 8u);                     // a column = two 16-byte halves: depth eq x0 x1 | x2 x3 del ins
    uint32_t lo = 0, range = k_hi - k_lo + 1, rank = len ? (len - 1) / 2 : 0;
    for (bool first = true; len > 0; first = false) {
        const uint32_t W = (range + AP_BINS - 1) / AP_BINS;
        for (int i = tid; i < AP_BINS; i += AP_SUM_THREADS) hist[i] = 0u;
        __syncthreads();
        uint32_t mn = 0xFFFFFFFFu, cont = 0;
        for (uint32_t j = tid; j < len; j += AP_SUM_THREADS) {
            const uint4 a = cols[2 * (size_t)j];
            const uint32_t depth = a.x;
            if (first) {
                const uint32_t ins = cols[2 * (size_t)j + 1].w;
                mn = min(mn, depth);
                cont += pu_contested(depth, a.y, ins) ? 1u : 0u;
            }
            if (depth >= lo && depth - lo < range) atomicAdd(&hist[(depth - lo) / W], 1u);
        }
        if (first) { atomicMin(&s_min, mn); if (cont) atomicAdd(&s_cont, cont); }
        __syncthreads();
        {
            uint32_t s = 0;
            for (int i = 0; i < AP_BINS / AP_SUM_THREADS; ++i) s += hist[tid * (AP_BINS / AP_SUM_THREADS) + i];
            part[tid] = s;
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t cum = 0; int g = 0;
            while (g < AP_SUM_THREADS - 1 && cum + part[g] <= rank) cum += part[g++];
            int b = g * (AP_BINS / AP_SUM_THREADS);
            while (b < AP_BINS - 1 && cum + hist[b] <= rank) cum += hist[b++];
            s_lo = lo + (uint32_t)b * W; s_k = rank - cum;
        }
        __syncthreads();
        lo = s_lo; rank = s_k;
        if (W == 1) break;
        range = W;
    }
    __syncthreads();
    if (tid == 0) {
        sp_support_summary sm;
        const uint32_t named = k_hi - k_lo;
        sm.n_members = n_members ? n_members[t] : named; sm.n_aligned = s_al; sm.n_unaligned = named - s_al; sm.length = len;
        sm.min_depth = len ? s_min : 0u; sm.median_depth = len ? lo : 0u; sm.n_contested = s_cont; sm.reserved_ = 0;
        out[t] = sm;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Insertion alleles (sp_pileup_ins; contract: include/starphase_hip.h, design: DESIGN.md section 7.2).  Five small kernels on one stream:
//   ins_collect   one wave per alignment walks its op row 64 ops at a time (the prefix sums of pu_pair); the lane of an 'I' op makes the run's record -- column, key,
//                 pair, query position -- and the wave appends its records to the run buffer (one ballot, one atomic on the cursor) and counts them per tile
//   ins_scan      one workgroup: exclusive sums of the tile counts
//   ins_scatter   every run to its tile's slice (a place from an atomic: the order inside a slice is whatever it is, the sort below makes it one order)
//   ins_tile      one workgroup per tile: sort the slice on (col, len, p0, p1, h, pair, qpos) -- a total order, (pair, qpos) is unique --, run-length compact it into
//                 distinct records (the first run of a record is its lowest pair), sort those into the list's order, fold the runs with a base outside ACGT (len 0)
//                 into n_other of their column's first record, write the tile's slice of the output
//   ins_pack      the slices back to back
// A run is listed behind the column pileup_rows_kernel counts it in (t0 - 1, when that is a column at all); the same pairs are skipped.
// ------------------------------------------------------------------------------------------------------------------------------
struct InsRun { uint64_t col, p0, p1, h; uint32_t len, pair, qpos, tile; };           // 48 bytes; len 0: a run with a base outside ACGT (p0 = p1 = h = 0)
static_assert(sizeof(InsRun) == 48 && sizeof(sp_pileup_ins) == 56, "record sizes");
constexpr int INS_THREADS = 256, INS_LDS_RUNS = SP_PILEUP_INS_LDS_RUNS;
constexpr uint64_t INS_FNV_BASIS = 0xcbf29ce484222325ull, INS_FNV_PRIME = 0x100000001b3ull;

__device__ __forceinline__ bool ins_same(const InsRun& a, const InsRun& b) { return a.col == b.col && a.len == b.len && a.p0 == b.p0 && a.p1 == b.p1 && a.h == b.h; }
__device__ __forceinline__ bool ins_run_less(const InsRun& a, const InsRun& b) {
    if (a.col != b.col) return a.col < b.col;
    if (a.len != b.len) return a.len < b.len;
    if (a.p0 != b.p0) return a.p0 < b.p0;
    if (a.p1 != b.p1) return a.p1 < b.p1;
    if (a.h != b.h) return a.h < b.h;
    if (a.pair != b.pair) return a.pair < b.pair;
    return a.qpos < b.qpos;
}

__global__ __launch_bounds__(INS_THREADS) void ins_collect_kernel(SeqSetView A, const int32_t* __restrict__ t_len, const sp_pair* __restrict__ pairs, const sp_affine_aln* __restrict__ aln,
                                                                  const uint32_t* __restrict__ n_cigar, const uint64_t* __restrict__ op_off, const uint32_t* __restrict__ ops, uint32_t n,
                                                                  uint32_t pair0, const uint64_t* __restrict__ col_offset, const uint32_t* __restrict__ tile_first,
                                                                  InsRun* __restrict__ runs, uint64_t runs_cap, unsigned long long* __restrict__ n_runs, uint32_t* __restrict__ tile_count) {
    const uint32_t i = blockIdx.x * (INS_THREADS / SP_WAVE) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & (SP_WAVE - 1);
    if (i >= n) return;                                                                 // (everything up to the loop is wave-uniform)
    const uint32_t n_ops = n_cigar[i];
    const uint64_t off = op_off[i];
    if (!ap_counted(n_ops, off, aln + i)) return;
    const sp_affine_aln g = aln[i];
    const sp_pair pr = pairs[i];
    const uint32_t* qwords = A.words + A.word_off[pr.a];
    const uint32_t* qn = A.nplane ? A.nplane + A.word_off[pr.a] : nullptr;
    const int tl_max = t_len[pr.b];
    pu_walk(ops + off, n_ops, g.b_start, g.a_start, lane, 0x7FFFFFFF, [&](bool live, uint32_t op, int len, int t0, int q0) {
        const bool is_ins = live && op == 1u && len > 0 && t0 - 1 >= 0 && t0 - 1 < tl_max;
        InsRun r;
        if (is_ins) {
            r.col = col_offset[pr.b] + (uint64_t)(t0 - 1); r.tile = tile_first[pr.b] + (uint32_t)(t0 - 1) / (uint32_t)PU_TILE;
            r.pair = pair0 + i; r.qpos = (uint32_t)q0; r.len = (uint32_t)len; r.p0 = 0; r.p1 = 0; r.h = INS_FNV_BASIS;
            bool other = false;
            for (int b = 0; b < len; ++b) {
                const int q = q0 + b;
                const uint64_t code = pu_query_code(qwords, q);
                if (qn && ((qn[q >> 4] >> ((q & 15) << 1)) & 3u)) other = true;
                if (b < 32) r.p0 |= code << (2 * b); else if (b < 64) r.p1 |= code << (2 * (b - 32));
                r.h = (r.h ^ code) * INS_FNV_PRIME;
            }
            if (other) { r.len = 0; r.p0 = 0; r.p1 = 0; r.h = 0; r.qpos = 0; r.pair = 0; }
        }
        const unsigned long long at = wave_append(is_ins, n_runs, lane);
        if (is_ins && at < runs_cap) { runs[at] = r; atomicAdd(&tile_count[r.tile], 1u); }
    });
}

// the workgroup's exclusive prefix of `mine` (part: INS_THREADS words of LDS); *total = the sum
__device__ __forceinline__ uint32_t ins_block_scan(uint32_t mine, uint32_t* part, uint32_t* total) {
    const uint32_t tid = threadIdx.x;
    __syncthreads();
    part[tid] = mine;
    __syncthreads();
    for (uint32_t d = 1; d < INS_THREADS; d <<= 1) {
        const uint32_t v = tid >= d ? part[tid - d] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    *total = part[INS_THREADS - 1];
    return part[tid] - mine;
}

// exclusive sums of cnt[0 .. n) into off[0 .. n], the total into off[n]; zero (optional): n words cleared on the way.  One workgroup.
__global__ __launch_bounds__(INS_THREADS) void ins_scan_kernel(const uint32_t* __restrict__ cnt, uint32_t n, uint32_t* __restrict__ off, uint32_t* __restrict__ zero) {
    __shared__ uint32_t part[INS_THREADS];
    const uint32_t tid = threadIdx.x, per = (n + INS_THREADS - 1) / INS_THREADS, lo = min(n, tid * per), hi = min(n, lo + per);
    uint32_t s = 0, total = 0;
    for (uint32_t j = lo; j < hi; ++j) s += cnt[j];
    uint32_t run = ins_block_scan(s, part, &total);
    for (uint32_t j = lo; j < hi; ++j) { off[j] = run; run += cnt[j]; if (zero) zero[j] = 0u; }
    if (tid == INS_THREADS - 1) off[n] = total;
}

__global__ void ins_scatter_kernel(const InsRun* __restrict__ runs, uint32_t n, const uint32_t* __restrict__ tile_off, uint32_t* __restrict__ tile_cur, InsRun* __restrict__ binned) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const InsRun r = runs[i];
    binned[tile_off[r.tile] + atomicAdd(&tile_cur[r.tile], 1u)] = r;
}

// v[0 .. n) = the numbers 0 .. n - 1 in ascending order of `less` (a total order on them), by the whole workgroup.  The bitonic network whose comparators all put the smaller element at the lower index (a merge
// begins with the mirrored step, then halves): for an n that is no power of two the places from n on stand for elements larger than all others, which such a
// comparator never moves -- a comparator that reaches past n is left out.
template <class Less> __device__ __forceinline__ void ins_bitonic(uint32_t* v, uint32_t n, Less less) {
    for (uint32_t s = threadIdx.x; s < n; s += INS_THREADS) v[s] = s;
    __syncthreads();
    uint32_t P = 1;
    while (P < n) P <<= 1;
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < P / 2; t += INS_THREADS) {
                const uint32_t blk = t / j, at = t % j;
                const uint32_t lo = (j == k >> 1) ? blk * k + at : blk * 2 * j + at, hi = (j == k >> 1) ? blk * k + k - 1 - at : lo + j;
                if (hi < n) {
                    const uint32_t a = v[lo], b = v[hi];
                    if (less(b, a)) { v[lo] = b; v[hi] = a; }
                }
            }
            __syncthreads();
        }
}

// The distinct records of the sorted idx[0 .. n), `same` telling whether two numbers belong to one record: didx[d] = the first number of record d in the order (the
// lowest of the record where the order ends on that), dcnt[d] = how many numbers the record has.  Returns the number of records.
template <class Same> __device__ __forceinline__ uint32_t ins_distinct(const uint32_t* idx, uint32_t* didx, uint32_t* dcnt, uint32_t n, uint32_t* part, Same same) {
    const uint32_t tid = threadIdx.x, per = (n + INS_THREADS - 1) / INS_THREADS, lo = min(n, tid * per), hi = min(n, lo + per);
    auto head = [&](uint32_t s) { return s == 0 || !same(idx[s], idx[s - 1]); };
    uint32_t heads = 0, m = 0;
    for (uint32_t s = lo; s < hi; ++s) heads += head(s) ? 1u : 0u;
    uint32_t d = ins_block_scan(heads, part, &m);
    for (uint32_t s = lo; s < hi; ++s) if (head(s)) didx[d++] = s;
    __syncthreads();
    for (uint32_t e = tid; e < m; e += INS_THREADS) dcnt[e] = (e + 1 < m ? didx[e + 1] : n) - didx[e];
    __syncthreads();
    for (uint32_t e = tid; e < m; e += INS_THREADS) didx[e] = idx[didx[e]];
    __syncthreads();
    return m;
}

// one tile's runs R[0 .. n) -> its records, in the list's order, to out; returns their number.  idx / didx / dcnt: n words each, where R lives (LDS or the pooled scratch).
__device__ __forceinline__ uint32_t ins_tile_work(const InsRun* R, uint32_t* idx, uint32_t* didx, uint32_t* dcnt, uint32_t n, uint32_t* part, sp_pileup_ins* __restrict__ out) {
    const uint32_t tid = threadIdx.x;
    ins_bitonic(idx, n, [&](uint32_t a, uint32_t b) { return ins_run_less(R[a], R[b]); });
    const uint32_t m = ins_distinct(idx, didx, dcnt, n, part, [&](uint32_t a, uint32_t b) { return ins_same(R[a], R[b]); });      // (a record's first run is its lowest pair)
    // ---- the list's order: col, a column's len-0 record first (it is folded away below), count descending, len, key
    ins_bitonic(idx, m, [&](uint32_t a, uint32_t b) {
        const InsRun& x = R[didx[a]]; const InsRun& y = R[didx[b]];
        if (x.col != y.col) return x.col < y.col;
        if ((x.len == 0) != (y.len == 0)) return x.len == 0;
        if (dcnt[a] != dcnt[b]) return dcnt[a] > dcnt[b];
        if (x.len != y.len) return x.len < y.len;
        if (x.p0 != y.p0) return x.p0 < y.p0;
        if (x.p1 != y.p1) return x.p1 < y.p1;
        return x.h < y.h;
    });
    // ---- a len-0 record with a neighbour behind it in its column leaves its count in that neighbour's n_other
    const uint32_t mper = (m + INS_THREADS - 1) / INS_THREADS, mlo = min(m, tid * mper), mhi = min(m, mlo + mper);
    auto dropped = [&](uint32_t e) { const InsRun& x = R[didx[idx[e]]]; return x.len == 0 && e + 1 < m && R[didx[idx[e + 1]]].col == x.col; };
    uint32_t kept = 0, total = 0;
    for (uint32_t e = mlo; e < mhi; ++e) kept += dropped(e) ? 0u : 1u;
    uint32_t at = ins_block_scan(kept, part, &total);
    for (uint32_t e = mlo; e < mhi; ++e) {
        if (dropped(e)) continue;
        const InsRun& x = R[didx[idx[e]]];
        sp_pileup_ins o;
        o.col = x.col; o.len = x.len; o.count = x.len ? dcnt[idx[e]] : 0u; o.p0 = x.p0; o.p1 = x.p1; o.h = x.h; o.first_pair = x.pair; o.first_qpos = x.qpos; o.reserved_ = 0;
        o.n_other = x.len == 0 ? dcnt[idx[e]] : (e > 0 && R[didx[idx[e - 1]]].len == 0 && R[didx[idx[e - 1]]].col == x.col) ? dcnt[idx[e - 1]] : 0u;
        out[at++] = o;
    }
    return total;
}

__global__ __launch_bounds__(INS_THREADS) void ins_tile_kernel(InsRun* __restrict__ binned, const uint32_t* __restrict__ tile_off, uint32_t* __restrict__ scratch, uint64_t scratch_stride,
                                                               sp_pileup_ins* __restrict__ tmp, uint32_t* __restrict__ n_dist) {
    __shared__ InsRun s_runs[INS_LDS_RUNS];
    __shared__ uint32_t s_idx[INS_LDS_RUNS], s_didx[INS_LDS_RUNS], s_dcnt[INS_LDS_RUNS], part[INS_THREADS];
    const uint32_t tile = blockIdx.x, b0 = tile_off[tile], n = tile_off[tile + 1] - b0;
    uint32_t m = 0;
    if (n == 0) { /* (uniform over the workgroup) */ }
    else if (n <= (uint32_t)INS_LDS_RUNS) {
        for (uint32_t s = threadIdx.x; s < n; s += INS_THREADS) s_runs[s] = binned[b0 + s];
        __syncthreads();
        m = ins_tile_work(s_runs, s_idx, s_didx, s_dcnt, n, part, tmp + b0);
    } else
        m = ins_tile_work(binned + b0, scratch + b0, scratch + scratch_stride + b0, scratch + 2 * scratch_stride + b0, n, part, tmp + b0);
    if (threadIdx.x == 0) n_dist[tile] = m;
}

__global__ void ins_pack_kernel(const sp_pileup_ins* __restrict__ tmp, const uint32_t* __restrict__ tile_off, const uint32_t* __restrict__ n_dist, const uint32_t* __restrict__ out_off,
                                sp_pileup_ins* __restrict__ out) {
    const uint32_t tile = blockIdx.x, n = n_dist[tile];
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) out[out_off[tile] + i] = tmp[tile_off[tile] + i];
}

// ------------------------------------------------------------------------------------------------------------------------------
// Read haplotypes (sp_support_hap; contract: include/starphase_hip.h, design: DESIGN.md section 7.2).  Behind the finished table, on one stream:
//   hap_cols      one workgroup per target: the first HAP_COLS contested columns (the rule of support_summary_kernel), ascending, and how many there are
//   hap_pattern   one wave per pair: the pair's calls at its target's listed columns, ORed into a 256-bit pattern in LDS, stored to pat[pair][4]; valid[pair] says
//                 whether the pair is one the table counts (the pairs pileup_rows_kernel skips are skipped)
//   hap_reduce    one workgroup per target: sort its (pattern, pair) keys -- a total order --, run-length compact them (the first key of a run is its lowest pair),
//                 sort the records by (count descending, pattern ascending), write them to the target's slice of a pooled output
//   hap_pack      the slices back to back, and the heads
// No global atomics: every word has one writer.
// ------------------------------------------------------------------------------------------------------------------------------
struct HapKey { uint64_t w[4]; uint32_t pair, valid; };                                // 40 bytes
static_assert(sizeof(HapKey) == 40 && sizeof(sp_support_hap) == 56 && sizeof(sp_support_hap_head) == 24, "record sizes");
constexpr int HAP_COLS = SP_SUPPORT_HAP_COLS, HAP_LDS_KEYS = SP_SUPPORT_HAP_LDS_KEYS, HAP_WAVES = INS_THREADS / SP_WAVE;
static_assert(HAP_COLS == 64 && HAP_WAVES == 4, "a pattern is 64 calls of 4 bits; hap_cols sums four waves");

__global__ __launch_bounds__(INS_THREADS) void hap_cols_kernel(const uint32_t* __restrict__ table, const uint64_t* __restrict__ col_offset, const int32_t* __restrict__ t_len,
                                                               uint32_t* __restrict__ list, uint32_t* __restrict__ ktot) {
    __shared__ uint32_t s_w[HAP_WAVES];
    const uint32_t t = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t len = (uint32_t)t_len[t];
    const uint4* cols = (const uint4*)(table + col_offset[t] * 8u);                     // a column = two 16-byte halves: depth eq x0 x1 | x2 x3 del ins
    uint32_t base = 0;                                                                  // contested columns in front of this chunk (uniform)
    for (uint32_t j0 = 0; j0 < len; j0 += INS_THREADS) {
        const uint32_t j = j0 + tid;
        bool c = false;
        if (j < len) {
            const uint4 a = cols[2 * (size_t)j];
            const uint32_t ins = cols[2 * (size_t)j + 1].w;
            c = pu_contested(a.x, a.y, ins);
        }
        const unsigned long long vote = __ballot(c);
        if (lane == 0) s_w[wave] = (uint32_t)__popcll(vote);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < (uint32_t)HAP_WAVES; ++w) { before += w < wave ? s_w[w] : 0u; total += s_w[w]; }
        if (c) {
            const uint32_t at = base + before + (uint32_t)__popcll(vote & ((1ull << lane) - 1ull));
            if (at < (uint32_t)HAP_COLS) list[(size_t)t * HAP_COLS + at] = j;
        }
        base += total;
        __syncthreads();
    }
    if (tid == 0) ktot[t] = base;
}

// first k in [0, K) with cols[k] >= c (K when there is none)
__device__ __forceinline__ int hap_lower(const uint32_t* cols, int K, uint32_t c) {
    int lo = 0, hi = K;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (cols[mid] < c) lo = mid + 1; else hi = mid; }
    return lo;
}

__global__ __launch_bounds__(INS_THREADS) void hap_pattern_kernel(SeqSetView A, const int32_t* __restrict__ t_len, const sp_pair* __restrict__ pairs, const sp_affine_aln* __restrict__ aln,
                                                                  const uint32_t* __restrict__ n_cigar, const uint64_t* __restrict__ op_off, const uint32_t* __restrict__ ops, uint32_t n,
                                                                  const uint32_t* __restrict__ list, const uint32_t* __restrict__ ktot,
                                                                  uint64_t* __restrict__ pat, uint32_t* __restrict__ valid) {
    __shared__ uint32_t s_cols[HAP_WAVES][HAP_COLS], s_pat[HAP_WAVES][8];
    const uint32_t wave = threadIdx.x >> 6, i = blockIdx.x * HAP_WAVES + wave;
    const int lane = threadIdx.x & (SP_WAVE - 1);
    // ---- everything the wave decides on is wave-uniform; the barriers are met by every wave of the workgroup
    bool act = i < n;
    uint32_t n_ops = 0; uint64_t off = 0; sp_affine_aln g = {}; sp_pair pr = {}; int K = 0;
    if (act) {
        n_ops = n_cigar[i]; off = op_off[i];
        act = ap_counted(n_ops, off, aln + i);
    }
    if (act) {
        g = aln[i]; pr = pairs[i];
        K = (int)min(ktot[pr.b], (uint32_t)HAP_COLS);
        if (lane < K) s_cols[wave][lane] = list[(size_t)pr.b * HAP_COLS + lane];
    }
    if (lane < 8) s_pat[wave][lane] = 0u;
    __syncthreads();
    if (act && K > 0) {
        const uint32_t* cols = s_cols[wave];
        uint32_t* mine = s_pat[wave];
        const uint32_t* qwords = A.words + A.word_off[pr.a];
        const int tl_max = t_len[pr.b], last = (int)cols[K - 1];
        // (an 'I' op at column last + 1 sits behind column last: the walk stops behind last + 1)
        pu_walk(ops + off, n_ops, g.b_start, g.a_start, lane, last + 1, [&](bool live, uint32_t op, int len, int t0, int q0) {
            const int tl = (op == 7u || op == 8u || op == 2u) ? len : 0;
            if (live && tl > 0) {
                for (int k = hap_lower(cols, K, (uint32_t)t0); k < K && (int)cols[k] < t0 + tl; ++k) {
                    const uint32_t call = op == 7u ? 1u : op == 2u ? 6u : 2u + pu_query_code(qwords, q0 + ((int)cols[k] - t0));
                    atomicOr(&mine[k >> 3], call << ((k & 7) << 2));
                }
            }
            if (live && op == 1u && t0 - 1 >= 0 && t0 - 1 < tl_max) {
                const int k = hap_lower(cols, K, (uint32_t)(t0 - 1));
                if (k < K && (int)cols[k] == t0 - 1) atomicOr(&mine[k >> 3], 8u << ((k & 7) << 2));
            }
        });
    }
    __syncthreads();
    if (i < n) {
        if (lane < 4) pat[(size_t)i * 4 + lane] = (uint64_t)s_pat[wave][2 * lane] | (uint64_t)s_pat[wave][2 * lane + 1] << 32;
        if (lane == 0) valid[i] = act ? 1u : 0u;
    }
}

__device__ __forceinline__ bool hap_same(const HapKey& a, const HapKey& b) { return a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2] && a.w[3] == b.w[3]; }
__device__ __forceinline__ bool hap_pat_less(const HapKey& a, const HapKey& b, bool* equal) {
    *equal = false;
    if (a.w[3] != b.w[3]) return a.w[3] < b.w[3];
    if (a.w[2] != b.w[2]) return a.w[2] < b.w[2];
    if (a.w[1] != b.w[1]) return a.w[1] < b.w[1];
    if (a.w[0] != b.w[0]) return a.w[0] < b.w[0];
    *equal = true;
    return false;
}

// one target's keys R[0 .. n) -> its records, in the list's order, to out; returns their number.  idx / didx / dcnt: n words each, where R lives (LDS or the pooled scratch).
__device__ __forceinline__ uint32_t hap_target_work(const HapKey* R, uint32_t* idx, uint32_t* didx, uint32_t* dcnt, uint32_t n, uint32_t* part, uint32_t target, uint32_t K,
                                                    sp_support_hap* __restrict__ out) {
    const uint32_t tid = threadIdx.x, per = (n + INS_THREADS - 1) / INS_THREADS, lo = min(n, tid * per), hi = min(n, lo + per);
    // the pairs the table does not count go behind all others; then the pattern, then the pair: a total order
    ins_bitonic(idx, n, [&](uint32_t a, uint32_t b) {
        const HapKey& x = R[a]; const HapKey& y = R[b];
        if (x.valid != y.valid) return x.valid > y.valid;
        bool eq;
        const bool less = hap_pat_less(x, y, &eq);
        return eq ? x.pair < y.pair : less;
    });
    uint32_t mine = 0, nv = 0;
    for (uint32_t s = lo; s < hi; ++s) mine += R[idx[s]].valid ? 1u : 0u;
    (void)ins_block_scan(mine, part, &nv);
    // ---- distinct records over the nv keys in front (a record's first key is its lowest pair)
    const uint32_t m = ins_distinct(idx, didx, dcnt, nv, part, [&](uint32_t a, uint32_t b) { return hap_same(R[a], R[b]); });
    // ---- the list's order: count descending, then the pattern ascending (distinct records have distinct patterns)
    ins_bitonic(idx, m, [&](uint32_t a, uint32_t b) {
        if (dcnt[a] != dcnt[b]) return dcnt[a] > dcnt[b];
        bool eq;
        return hap_pat_less(R[didx[a]], R[didx[b]], &eq);
    });
    for (uint32_t e = tid; e < m; e += INS_THREADS) {
        const HapKey& x = R[didx[idx[e]]];
        sp_support_hap o;
        o.target = target; o.n_cols = K; o.count = dcnt[idx[e]]; o.first_pair = x.pair; o.reserved_ = 0;
        o.w[0] = x.w[0]; o.w[1] = x.w[1]; o.w[2] = x.w[2]; o.w[3] = x.w[3];
        out[e] = o;
    }
    return m;
}

__global__ __launch_bounds__(INS_THREADS) void hap_reduce_kernel(const uint64_t* __restrict__ pat, const uint32_t* __restrict__ valid, const uint32_t* __restrict__ order,
                                                                 const uint32_t* __restrict__ boff, uint32_t n_slices, const uint32_t* __restrict__ ktot, HapKey* __restrict__ keys,
                                                                 uint32_t* __restrict__ scratch, uint64_t scratch_stride, sp_support_hap* __restrict__ tmp, uint32_t* __restrict__ n_dist) {
    __shared__ HapKey s_keys[HAP_LDS_KEYS];
    __shared__ uint32_t s_idx[HAP_LDS_KEYS], s_didx[HAP_LDS_KEYS], s_dcnt[HAP_LDS_KEYS], part[INS_THREADS];
    const uint32_t t = blockIdx.x, k_lo = boff[(size_t)t * (n_slices + 1)], n = boff[(size_t)t * (n_slices + 1) + n_slices] - k_lo;
    const uint32_t K = min(ktot[t], (uint32_t)HAP_COLS);
    uint32_t m = 0;
    if (n > 0 && K > 0) {                                                              // (uniform over the workgroup)
        const bool in_lds = n <= (uint32_t)HAP_LDS_KEYS;
        HapKey* R = in_lds ? s_keys : keys + k_lo;
        for (uint32_t s = threadIdx.x; s < n; s += INS_THREADS) {
            const uint32_t p = order[k_lo + s];
            HapKey k;
            k.w[0] = pat[(size_t)p * 4]; k.w[1] = pat[(size_t)p * 4 + 1]; k.w[2] = pat[(size_t)p * 4 + 2]; k.w[3] = pat[(size_t)p * 4 + 3]; k.pair = p; k.valid = valid[p];
            R[s] = k;
        }
        __syncthreads();
        if (in_lds) m = hap_target_work(R, s_idx, s_didx, s_dcnt, n, part, t, K, tmp + k_lo);
        else m = hap_target_work(R, scratch + k_lo, scratch + scratch_stride + k_lo, scratch + 2 * scratch_stride + k_lo, n, part, t, K, tmp + k_lo);
    }
    if (threadIdx.x == 0) n_dist[t] = m;
}

__global__ void hap_pack_kernel(const sp_support_hap* __restrict__ tmp, const uint32_t* __restrict__ boff, uint32_t n_slices, const uint32_t* __restrict__ n_dist,
                                const uint32_t* __restrict__ out_off, const uint32_t* __restrict__ ktot, sp_support_hap* __restrict__ out, sp_support_hap_head* __restrict__ heads) {
    const uint32_t t = blockIdx.x, n = n_dist[t], k_lo = boff[(size_t)t * (n_slices + 1)];
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) out[out_off[t] + i] = tmp[k_lo + i];
    if (threadIdx.x == 0) {
        sp_support_hap_head h;
        h.first_record = out_off[t]; h.n_records = n; h.n_cols = min(ktot[t], (uint32_t)HAP_COLS); h.n_cols_total = ktot[t]; h.reserved_ = 0;
        heads[t] = h;
    }
}

static int32_t check_col_offset(sp_ctx* ctx, const std::string& who, const sp_seqset* B, const uint64_t* col_offset) {
    if (col_offset[0] != 0) return sp_fail(ctx, SP_ERR_INVALID_ARG, who + ": col_offset[0] must be 0");
    for (uint32_t t = 0; t < B->n; ++t)
        if (col_offset[t + 1] < col_offset[t] || col_offset[t + 1] - col_offset[t] != (uint64_t)B->h_len[t]) return sp_fail(ctx, SP_ERR_INVALID_ARG, who + ": col_offset does not follow the target lengths");
    return SP_OK;
}

// the tiles of B's targets: how many a target of `len` columns has, how many there are in all (more than 2^31 - 1: an error), and the list in target order
static uint64_t pu_tiles_of(int32_t len) { return ((uint64_t)len + PU_TILE - 1) / PU_TILE; }
static int32_t pu_count_tiles(sp_ctx* ctx, const std::string& who, const sp_seqset* B, uint64_t* n_tiles) {
    *n_tiles = 0;
    for (uint32_t t = 0; t < B->n; ++t) *n_tiles += pu_tiles_of(B->h_len[t]);
    return *n_tiles > 0x7FFFFFFFull ? sp_fail(ctx, SP_ERR_INVALID_ARG, who + ": too many tiles") : SP_OK;
}
static void pu_fill_tiles(const sp_seqset* B, PuTile* list) {
    for (uint32_t t = 0; t < B->n; ++t) for (int32_t c0 = 0; c0 < B->h_len[t]; c0 += PU_TILE) *list++ = PuTile{ t, (uint32_t)c0 };
}

// ---- the host side of the insertion list: pooled buffers sized by the run buffer's capacity (a warm context allocates nothing), the launches, the way out
struct InsPass {
    uint64_t cap = 0; uint32_t n_tiles = 0, n_t = 0;
    InsRun* d_runs = nullptr; InsRun* d_binned = nullptr; sp_pileup_ins* d_tmp = nullptr; uint32_t* d_scratch = nullptr;
    unsigned long long* d_n = nullptr; uint32_t *d_cnt = nullptr, *d_off = nullptr, *d_cur = nullptr, *d_ooff = nullptr, *d_tfirst = nullptr;
    uint64_t* h_st = nullptr;
};

// min_cap: the runs the caller knows of (0: a guess from the number of pairs; the pass is run again when it was too small)
static int32_t ins_begin(sp_ctx* ctx, const std::string& who, const sp_seqset* B, uint64_t n_pairs, uint64_t min_cap, InsPass* ip) {
    ip->n_t = B->n;
    uint64_t n_tiles = 0;
    const int32_t rc = pu_count_tiles(ctx, who, B, &n_tiles);
    if (rc != SP_OK) return rc;
    ip->n_tiles = (uint32_t)n_tiles;
    const uint64_t held = std::min(std::min<uint64_t>(sp_pool_bytes(ctx, "ins_runs") / sizeof(sp_pileup_ins), sp_pool_bytes(ctx, "ins_binned") / sizeof(InsRun)),
                                   std::min<uint64_t>(sp_pool_bytes(ctx, "ins_tmp") / sizeof(sp_pileup_ins), sp_pool_bytes(ctx, "ins_scratch") / 12));
    ip->cap = std::max<uint64_t>(held, min_cap ? min_cap : 1024 + 4 * n_pairs);
    if (ip->cap > 0x7FFFFFFFull) /* (ins_bitonic rounds a tile's runs up to a power of two in 32 bits) */ return sp_fail(ctx, SP_ERR_CAPACITY, who + ": more insertion runs than the list counts");
    const size_t tw = (size_t)n_tiles + 1, words = 4 + 4 * tw + (size_t)B->n + 1;
    ip->d_runs = (InsRun*)sp_pool(ctx, "ins_runs", (size_t)ip->cap * sizeof(sp_pileup_ins));          // (the packed list takes the runs' place once they are binned)
    ip->d_binned = (InsRun*)sp_pool(ctx, "ins_binned", (size_t)ip->cap * sizeof(InsRun));
    ip->d_tmp = (sp_pileup_ins*)sp_pool(ctx, "ins_tmp", (size_t)ip->cap * sizeof(sp_pileup_ins));
    ip->d_scratch = (uint32_t*)sp_pool(ctx, "ins_scratch", (size_t)ip->cap * 12);
    uint32_t* d_w = (uint32_t*)sp_pool(ctx, "ins_tiles", words * 4);
    uint32_t* h_tf = (uint32_t*)sp_host_pool(ctx, "ins_tiles", ((size_t)B->n + 1) * 4);
    ip->h_st = (uint64_t*)sp_host_pool(ctx, "ins_st", 16);
    if (!ip->d_runs || !ip->d_binned || !ip->d_tmp || !ip->d_scratch || !d_w || !h_tf || !ip->h_st) return sp_fail(ctx, SP_ERR_OUT_OF_MEMORY, who + ": insertion list buffers");
    ip->d_n = (unsigned long long*)d_w; ip->d_cnt = d_w + 4; ip->d_off = ip->d_cnt + tw; ip->d_cur = ip->d_off + tw; ip->d_ooff = ip->d_cur + tw; ip->d_tfirst = ip->d_ooff + tw;
    uint32_t x = 0;
    for (uint32_t t = 0; t < B->n; ++t) { h_tf[t] = x; x += (uint32_t)pu_tiles_of(B->h_len[t]); }
    h_tf[B->n] = x;
    SP_HIP_CHECK(ctx, hipMemsetAsync(d_w, 0, (4 + 4 * tw) * 4, ctx->stream));
    SP_HIP_CHECK(ctx, hipMemcpyAsync(ip->d_tfirst, h_tf, ((size_t)B->n + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    return SP_OK;
}

// the runs of m alignments (pair numbers pair0 ...) whose rows lie in device memory
static int32_t ins_collect(sp_ctx* ctx, const std::string& who, const InsPass& ip, const sp_seqset* A, const sp_seqset* B, const sp_pair* d_pairs, const sp_affine_aln* d_aln,
                           const uint32_t* d_nc, const uint64_t* d_op_off, const uint32_t* d_ops, uint32_t m, uint32_t pair0, const uint64_t* d_col_offset) {
    if (m == 0 || ip.n_tiles == 0) return SP_OK;
    ProfScope ps(ctx, "pileup_ins_collect", m);
    constexpr uint32_t per = INS_THREADS / SP_WAVE;
    hipLaunchKernelGGL(ins_collect_kernel, dim3((m + per - 1) / per), dim3(INS_THREADS), 0, ctx->stream, A->view(), B->d_len, d_pairs, d_aln, d_nc, d_op_off, d_ops, m, pair0,
                       d_col_offset, ip.d_tfirst, ip.d_runs, ip.cap, ip.d_n, ip.d_cnt);
    if (hipGetLastError() != hipSuccess) return sp_fail(ctx, SP_ERR_HIP, who + ": insertion collect launch failed");
    return SP_OK;
}

// everything behind the last collect.  *grow != 0 on return: the run buffer was too small for that many runs, nothing was written -- run the pass again.
static int32_t ins_finish(sp_ctx* ctx, const std::string& who, const InsPass& ip, sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins, uint64_t* grow) {
    *grow = 0; *n_ins = 0;
    if (ip.n_tiles == 0) return SP_OK;
    SP_HIP_CHECK(ctx, hipMemcpyAsync(ip.h_st, ip.d_n, 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t n_runs = ip.h_st[0];
    if (n_runs > ip.cap) { *grow = n_runs; return SP_OK; }
    if (n_runs == 0) return SP_OK;
    const uint32_t N = (uint32_t)n_runs;
    sp_pileup_ins* d_out = (sp_pileup_ins*)ip.d_runs;
    {
        ProfScope ps(ctx, "pileup_ins_reduce", n_runs);
        hipLaunchKernelGGL(ins_scan_kernel, dim3(1), dim3(INS_THREADS), 0, ctx->stream, ip.d_cnt, ip.n_tiles, ip.d_off, ip.d_cur);
        hipLaunchKernelGGL(ins_scatter_kernel, dim3((N + 255) / 256), dim3(256), 0, ctx->stream, ip.d_runs, N, ip.d_off, ip.d_cur, ip.d_binned);
        hipLaunchKernelGGL(ins_tile_kernel, dim3(ip.n_tiles), dim3(INS_THREADS), 0, ctx->stream, ip.d_binned, ip.d_off, ip.d_scratch, ip.cap, ip.d_tmp, ip.d_cur);
        hipLaunchKernelGGL(ins_scan_kernel, dim3(1), dim3(INS_THREADS), 0, ctx->stream, ip.d_cur, ip.n_tiles, ip.d_ooff, (uint32_t*)nullptr);
        hipLaunchKernelGGL(ins_pack_kernel, dim3(ip.n_tiles), dim3(256), 0, ctx->stream, ip.d_tmp, ip.d_off, ip.d_cur, ip.d_ooff, d_out);
        if (hipGetLastError() != hipSuccess) return sp_fail(ctx, SP_ERR_HIP, who + ": insertion list launch failed");
    }
    uint32_t* h_total = (uint32_t*)(ip.h_st + 1);
    SP_HIP_CHECK(ctx, hipMemcpyAsync(h_total, ip.d_ooff + ip.n_tiles, 4, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    *n_ins = *h_total;
    if (*n_ins > ins_cap) return sp_fail(ctx, SP_ERR_CAPACITY, who + ": " + std::to_string(*n_ins) + " insertion records, room for " + std::to_string(ins_cap));
    SP_HIP_CHECK(ctx, hipMemcpyAsync(ins, d_out, (size_t)*n_ins * sizeof(sp_pileup_ins), hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
}

// Every alignment of host op rows is walked here, before anything is launched or written: what the kernels index with is what this loop has seen.  *total_ops
// counts the ops of the pairs that have any, *n_ins_ops the 'I' ops among them.
static int32_t pileup_check_rows(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_aln* aln, const uint32_t* cigar,
                                 uint32_t cigar_stride, const uint32_t* n_cigar, uint64_t* total_ops, uint64_t* n_ins_ops) {
    for (uint64_t i = 0; i < n_pairs; ++i) {
        if (pairs[i].a >= A->n || pairs[i].b >= B->n) return sp_fail(ctx, SP_ERR_INVALID_ARG, "pileup: index out of range");
        if (n_cigar[i] == 0) continue;
        const std::string who = "pileup: pair " + std::to_string(i);
        if (n_cigar[i] > cigar_stride || !cigar) return sp_fail(ctx, SP_ERR_INVALID_ARG, who + " has more ops than its row holds");
        const sp_affine_aln& g = aln[i];
        if (g.b_start < 0 || g.b_end < g.b_start || g.b_end > B->h_len[pairs[i].b] || g.a_start < 0 || g.a_end < g.a_start || g.a_end > A->h_len[pairs[i].a])
            return sp_fail(ctx, SP_ERR_INVALID_ARG, who + ": spans outside the sequences");
        int64_t j = g.b_start, q = g.a_start;
        const uint32_t* row = cigar + i * (size_t)cigar_stride;
        for (uint32_t k = 0; k < n_cigar[i]; ++k) {
            const uint32_t op = row[k] & 15u; const int64_t n = (int64_t)(row[k] >> 4);
            if (n == 0) return sp_fail(ctx, SP_ERR_INVALID_ARG, who + ": a run of length 0");
            if (op == 7u || op == 8u) { j += n; q += n; }
            else if (op == 2u) j += n;
            else if (op == 1u) { if (j == g.b_start) return sp_fail(ctx, SP_ERR_INVALID_ARG, who + ": an insertion before the first target column"); q += n; ++*n_ins_ops; }
            else return sp_fail(ctx, SP_ERR_INVALID_ARG, who + ": an op other than = X I D");
            if (j > g.b_end || q > g.a_end) return sp_fail(ctx, SP_ERR_INVALID_ARG, who + ": the ops do not consume the spans of its alignment");
        }
        if (j != g.b_end || q != g.a_end) return sp_fail(ctx, SP_ERR_INVALID_ARG, who + ": the ops do not consume the spans of its alignment");
        *total_ops += n_cigar[i];
    }
    return SP_OK;
}

// the two tile kernels take more dynamic LDS than the 64 KiB a kernel gets unasked: said once per device of the process
static int32_t pileup_lds(sp_ctx* ctx) {
    static std::atomic<uint64_t> lds_set(0);
    const uint64_t bit = 1ull << (ctx->device & 63);
    if (!(lds_set.load() & bit)) {
        SP_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)pileup_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PU_LDS_BYTES));
        SP_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)pileup_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PU_LDS_BYTES));
        lds_set.fetch_or(bit);
    }
    return SP_OK;
}

// Host op rows (checked by pileup_check_rows) as the device-resident pass keeps them, in one staging block and one copy: the pair list, spans, op counts and op offsets
// per pair, the column offsets, the ops back to back; with_table also the order and the offsets of ONE slice, the tiles, and the table's buffer.  The kernels skip
// score <= 0 (ap_counted) where the host-row entry points count every pair with ops: the staged spans of those carry score 1.
struct HostRows {
    const sp_pair* pairs; const sp_affine_aln* aln; const uint32_t *nc, *ops, *order, *boff; const uint64_t *off, *cols; const PuTile* tiles;
    uint64_t n_tiles; uint32_t* table;
};

static int32_t stage_rows(sp_ctx* ctx, const sp_seqset* B, const sp_pair* pairs, uint32_t n, const sp_affine_aln* aln, const uint32_t* cigar, uint32_t cigar_stride,
                          const uint32_t* n_cigar, const uint64_t* col_offset, uint64_t total_ops, bool with_table, HostRows* hr, bool order_only = false) {
    const uint32_t n_t = B->n;
    const bool with_order = with_table || order_only;                                     // (order_only: the order and the offsets without tiles and table -- the window kernel)
    hr->n_tiles = 0; hr->table = nullptr;
    if (with_table) {
        const int32_t rc = pu_count_tiles(ctx, "pileup", B, &hr->n_tiles);
        if (rc != SP_OK) return rc;
    }
    (void)hipSetDevice(ctx->device);
    const size_t n_ord = with_order ? n : 0, n_boff = with_order ? (size_t)n_t * 2 + 1 : 0;
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t at_pairs = 0, at_aln = up16(at_pairs + sizeof(sp_pair) * (size_t)n), at_nc = up16(at_aln + sizeof(sp_affine_aln) * (size_t)n), at_off = up16(at_nc + 4 * (size_t)n),
                 at_order = up16(at_off + 8 * (size_t)n), at_boff = up16(at_order + 4 * n_ord), at_tiles = up16(at_boff + 4 * n_boff),
                 at_cols = up16(at_tiles + sizeof(PuTile) * (size_t)hr->n_tiles), at_ops = up16(at_cols + 8 * ((size_t)n_t + 1)), in_bytes = up16(at_ops + 4 * (size_t)total_ops) + 16;
    uint8_t* h_in = (uint8_t*)sp_host_pool(ctx, "pileup_in", in_bytes);
    uint8_t* d_in = (uint8_t*)sp_pool(ctx, "pileup_in", in_bytes);
    if (with_table) hr->table = (uint32_t*)sp_pool(ctx, "pileup_out", std::max<size_t>(16, col_offset[n_t] * sizeof(sp_pileup_col)));
    if (!h_in || !d_in || (with_table && !hr->table)) return sp_fail(ctx, SP_ERR_OUT_OF_MEMORY, "pileup buffers");
    if (n) std::memcpy(h_in + at_pairs, pairs, sizeof(sp_pair) * (size_t)n);
    if (n) std::memcpy(h_in + at_nc, n_cigar, 4 * (size_t)n);
    std::memcpy(h_in + at_cols, col_offset, 8 * ((size_t)n_t + 1));
    sp_affine_aln* ha = (sp_affine_aln*)(h_in + at_aln);
    uint64_t* hoff = (uint64_t*)(h_in + at_off); uint32_t* hops = (uint32_t*)(h_in + at_ops);
    uint64_t op_at = 0;
    for (uint32_t i = 0; i < n; ++i) {
        ha[i] = aln[i]; hoff[i] = op_at;
        if (n_cigar[i] == 0) continue;
        ha[i].score = 1;
        std::memcpy(hops + op_at, cigar + i * (size_t)cigar_stride, 4 * (size_t)n_cigar[i]);
        op_at += n_cigar[i];
    }
    if (with_order) {
        // target t's pairs are order[boff[2 t] .. boff[2 t + 1]), in the order given (pileup_rows_kernel with n_slices = 1)
        uint32_t* boff = (uint32_t*)(h_in + at_boff); uint32_t* hord = (uint32_t*)(h_in + at_order);
        std::memset(boff, 0, 4 * n_boff);
        for (uint32_t i = 0; i < n; ++i) ++boff[(size_t)pairs[i].b * 2 + 1];
        uint32_t run = 0;
        for (uint32_t t = 0; t < n_t; ++t) { boff[(size_t)t * 2] = run; run += boff[(size_t)t * 2 + 1]; boff[(size_t)t * 2 + 1] = run; }
        std::vector<uint32_t> at(n_t);
        for (uint32_t t = 0; t < n_t; ++t) at[t] = boff[(size_t)t * 2];
        for (uint32_t i = 0; i < n; ++i) hord[at[pairs[i].b]++] = i;
        if (with_table) pu_fill_tiles(B, (PuTile*)(h_in + at_tiles));
    }
    SP_HIP_CHECK(ctx, hipMemcpyAsync(d_in, h_in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    hr->pairs = (const sp_pair*)(d_in + at_pairs); hr->aln = (const sp_affine_aln*)(d_in + at_aln); hr->nc = (const uint32_t*)(d_in + at_nc); hr->off = (const uint64_t*)(d_in + at_off);
    hr->ops = (const uint32_t*)(d_in + at_ops); hr->order = (const uint32_t*)(d_in + at_order); hr->boff = (const uint32_t*)(d_in + at_boff);
    hr->tiles = (const PuTile*)(d_in + at_tiles); hr->cols = (const uint64_t*)(d_in + at_cols);
    return SP_OK;
}

// ---- the host side of the haplotype list (HapOut: sp_internal.h): one pooled buffer carved by the numbers of pairs and targets (a warm context allocates nothing), the
// launches, the way out.  The list over n pairs whose rows lie in device memory (d_ops: the rows of ALL of them), behind the finished table d_table.  A list that does not fit: SP_ERR_CAPACITY,
// *n_haps set, nothing written.
static int32_t hap_run(sp_ctx* ctx, const std::string& who, const sp_seqset* A, const sp_seqset* B, uint32_t n, const uint32_t* d_table, const uint64_t* d_col_offset,
                       const sp_pair* d_pairs, const sp_affine_aln* d_aln, const uint32_t* d_nc, const uint64_t* d_op_off, const uint32_t* d_ops,
                       const uint32_t* d_order, const uint32_t* d_boff, uint32_t n_slices, const HapOut& ho) {
    const uint32_t n_t = B->n;
    *ho.n_haps = 0;
    if (n_t == 0) return SP_OK;
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t np = std::max<size_t>(n, 1);
    const size_t at_list = 0, at_ktot = up16(at_list + 4 * (size_t)n_t * HAP_COLS), at_ndist = up16(at_ktot + 4 * (size_t)n_t), at_ooff = up16(at_ndist + 4 * (size_t)n_t),
                 at_valid = up16(at_ooff + 4 * ((size_t)n_t + 1)), at_scratch = up16(at_valid + 4 * np), at_pat = up16(at_scratch + 12 * np), at_keys = up16(at_pat + 32 * np),
                 at_tmp = up16(at_keys + sizeof(HapKey) * np), at_out = up16(at_tmp + sizeof(sp_support_hap) * np), at_heads = up16(at_out + sizeof(sp_support_hap) * np),
                 bytes = up16(at_heads + sizeof(sp_support_hap_head) * (size_t)n_t);
    uint8_t* d = (uint8_t*)sp_pool(ctx, "hap", bytes);
    uint32_t* h_total = (uint32_t*)sp_host_pool(ctx, "hap_st", 16);
    if (!d || !h_total) return sp_fail(ctx, SP_ERR_OUT_OF_MEMORY, who + ": haplotype list buffers");
    uint32_t *d_list = (uint32_t*)(d + at_list), *d_ktot = (uint32_t*)(d + at_ktot), *d_ndist = (uint32_t*)(d + at_ndist), *d_ooff = (uint32_t*)(d + at_ooff);
    uint32_t *d_valid = (uint32_t*)(d + at_valid), *d_scratch = (uint32_t*)(d + at_scratch);
    uint64_t* d_pat = (uint64_t*)(d + at_pat); HapKey* d_keys = (HapKey*)(d + at_keys);
    sp_support_hap *d_tmp = (sp_support_hap*)(d + at_tmp), *d_out = (sp_support_hap*)(d + at_out);
    sp_support_hap_head* d_heads = (sp_support_hap_head*)(d + at_heads);
    {
        ProfScope ps(ctx, "support_hap", n);
        hipLaunchKernelGGL(hap_cols_kernel, dim3(n_t), dim3(INS_THREADS), 0, ctx->stream, d_table, d_col_offset, B->d_len, d_list, d_ktot);
        if (n) hipLaunchKernelGGL(hap_pattern_kernel, dim3((n + HAP_WAVES - 1) / HAP_WAVES), dim3(INS_THREADS), 0, ctx->stream, A->view(), B->d_len, d_pairs, d_aln, d_nc, d_op_off, d_ops, n,
                                  d_list, d_ktot, d_pat, d_valid);
        hipLaunchKernelGGL(hap_reduce_kernel, dim3(n_t), dim3(INS_THREADS), 0, ctx->stream, d_pat, d_valid, d_order, d_boff, n_slices, d_ktot, d_keys, d_scratch, (uint64_t)np, d_tmp, d_ndist);
        hipLaunchKernelGGL(ins_scan_kernel, dim3(1), dim3(INS_THREADS), 0, ctx->stream, d_ndist, n_t, d_ooff, (uint32_t*)nullptr);
        hipLaunchKernelGGL(hap_pack_kernel, dim3(n_t), dim3(256), 0, ctx->stream, d_tmp, d_boff, n_slices, d_ndist, d_ooff, d_ktot, d_out, d_heads);
        if (hipGetLastError() != hipSuccess) return sp_fail(ctx, SP_ERR_HIP, who + ": haplotype list launch failed");
    }
    SP_HIP_CHECK(ctx, hipMemcpyAsync(h_total, d_ooff + n_t, 4, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    *ho.n_haps = *h_total;
    if (*ho.n_haps > ho.cap) return sp_fail(ctx, SP_ERR_CAPACITY, who + ": " + std::to_string(*ho.n_haps) + " haplotype records, room for " + std::to_string(ho.cap));
    if (*ho.n_haps) SP_HIP_CHECK(ctx, hipMemcpyAsync(ho.haps, d_out, (size_t)*ho.n_haps * sizeof(sp_support_hap), hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP_CHECK(ctx, hipMemcpyAsync(ho.heads, d_heads, (size_t)n_t * sizeof(sp_support_hap_head), hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
}

// ---- the host side of window support: the windows checked (before anything is launched), the chunk list, their part of a staging block, the launch of one slice
struct WinStage { uint64_t n_w = 0, n_chunks = 0; size_t at_off = 0, at_chunks = 0, at_wins = 0, end = 0; };

// from: where the part begins in the staging block (16-byte aligned); without windows the part is empty and ws->end == from
static int32_t win_plan(sp_ctx* ctx, const std::string& who, const sp_seqset* B, const WinIn* win, size_t from, WinStage* ws) {
    *ws = WinStage(); ws->at_off = ws->at_chunks = ws->at_wins = ws->end = from;
    if (!win) return SP_OK;
    const uint32_t n_t = B->n;
    if (!win->win_offset || win->win_offset[0] != 0) return sp_fail(ctx, SP_ERR_INVALID_ARG, who + ": win_offset must begin at 0");
    for (uint32_t t = 0; t < n_t; ++t) if (win->win_offset[t + 1] < win->win_offset[t]) return sp_fail(ctx, SP_ERR_INVALID_ARG, who + ": win_offset does not ascend");
    ws->n_w = win->win_offset[n_t];
    if (ws->n_w > 0x7FFFFFFFull) return sp_fail(ctx, SP_ERR_INVALID_ARG, who + ": too many windows");
    if (ws->n_w && (!win->windows || !win->out)) return sp_fail(ctx, SP_ERR_INVALID_ARG, who + ": null argument");
    for (uint32_t t = 0; t < n_t; ++t) {
        for (uint64_t i = win->win_offset[t]; i < win->win_offset[t + 1]; ++i)
            if (win->windows[i].start >= win->windows[i].end || win->windows[i].end > (uint32_t)B->h_len[t])
                return sp_fail(ctx, SP_ERR_INVALID_ARG, who + ": window " + std::to_string(i) + " is empty or leaves its target");
        ws->n_chunks += (win->win_offset[t + 1] - win->win_offset[t] + WIN_CHUNK - 1) / WIN_CHUNK;
    }
    if (ws->n_w == 0) return SP_OK;
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    ws->at_off = from; ws->at_chunks = up16(ws->at_off + 4 * ((size_t)n_t + 1)); ws->at_wins = up16(ws->at_chunks + sizeof(WinChunk) * (size_t)ws->n_chunks);
    ws->end = up16(ws->at_wins + sizeof(sp_window) * (size_t)ws->n_w);
    return SP_OK;
}

static void win_fill(const WinStage& ws, uint8_t* h_in, const sp_seqset* B, const WinIn* win) {
    if (ws.n_w == 0) return;
    uint32_t* off = (uint32_t*)(h_in + ws.at_off); WinChunk* ch = (WinChunk*)(h_in + ws.at_chunks);
    for (uint32_t t = 0; t <= B->n; ++t) off[t] = (uint32_t)win->win_offset[t];
    for (uint32_t t = 0; t < B->n; ++t) for (uint32_t w0 = 0; w0 < off[t + 1] - off[t]; w0 += WIN_CHUNK) *ch++ = WinChunk{ t, w0 };
    std::memcpy(h_in + ws.at_wins, win->windows, sizeof(sp_window) * (size_t)ws.n_w);
}

// one slice's pairs under every chunk; d_in: the staging block on the device
static int32_t win_launch(sp_ctx* ctx, const std::string& who, const WinStage& ws, const uint8_t* d_in, const sp_affine_aln* d_aln, const uint32_t* d_nc, const uint64_t* d_op_off,
                          const uint32_t* d_ops, const uint32_t* d_order, const uint32_t* d_boff, uint32_t n_slices, uint32_t slice, sp_window_support* d_out) {
    if (ws.n_chunks == 0) return SP_OK;
    ProfScope ps(ctx, "pileup_windows", ws.n_w);
    hipLaunchKernelGGL(window_kernel, dim3((unsigned)ws.n_chunks), dim3(WIN_WAVES * SP_WAVE), 0, ctx->stream, d_aln, d_nc, d_op_off, d_ops, d_order, d_boff, n_slices, slice,
                       (const WinChunk*)(d_in + ws.at_chunks), (const uint32_t*)(d_in + ws.at_off), (const sp_window*)(d_in + ws.at_wins), d_out);
    if (hipGetLastError() != hipSuccess) return sp_fail(ctx, SP_ERR_HIP, who + ": window launch failed");
    return SP_OK;
}

} // namespace

extern "C" {

int32_t sp_pileup_windows_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_aln* aln,
                                const uint32_t* cigar, uint32_t cigar_stride, const uint32_t* n_cigar, const uint64_t* col_offset,
                                const uint64_t* win_offset, const sp_window* windows, sp_window_support* out) {
    if (!ctx) return SP_ERR_INVALID_ARG;
    if (!A || !B || !col_offset || !win_offset || (n_pairs && (!pairs || !aln || !n_cigar))) return sp_fail(ctx, SP_ERR_INVALID_ARG, "pileup: null argument");
    if (n_pairs > 0x7FFFFFFFull) return sp_fail(ctx, SP_ERR_INVALID_ARG, "pileup: too many pairs");
    int32_t rc = check_col_offset(ctx, "pileup", B, col_offset);
    if (rc != SP_OK) return rc;
    uint64_t total_ops = 0, n_ins_ops = 0;
    rc = pileup_check_rows(ctx, A, B, pairs, n_pairs, aln, cigar, cigar_stride, n_cigar, &total_ops, &n_ins_ops);
    if (rc != SP_OK) return rc;
    const WinIn win = { win_offset, windows, out };
    WinStage ws;
    rc = win_plan(ctx, "pileup", B, &win, 0, &ws);
    if (rc != SP_OK || ws.n_w == 0) return rc;
    HostRows hr;
    rc = stage_rows(ctx, B, pairs, (uint32_t)n_pairs, aln, cigar, cigar_stride, n_cigar, col_offset, total_ops, false, &hr, true);
    if (rc != SP_OK) return rc;
    uint8_t* h_w = (uint8_t*)sp_host_pool(ctx, "pileup_win_in", ws.end);
    uint8_t* d_w = (uint8_t*)sp_pool(ctx, "pileup_win_in", ws.end);
    sp_window_support* d_out = (sp_window_support*)sp_pool(ctx, "pileup_win_out", (size_t)ws.n_w * sizeof(sp_window_support));
    if (!h_w || !d_w || !d_out) return sp_fail(ctx, SP_ERR_OUT_OF_MEMORY, "pileup buffers");
    win_fill(ws, h_w, B, &win);
    SP_HIP_CHECK(ctx, hipMemcpyAsync(d_w, h_w, ws.end, hipMemcpyHostToDevice, ctx->stream));
    rc = win_launch(ctx, "pileup", ws, d_w, hr.aln, hr.nc, hr.off, hr.ops, hr.order, hr.boff, 1, 0, d_out);
    if (rc != SP_OK) return rc;
    SP_HIP_CHECK(ctx, hipMemcpyAsync(out, d_out, (size_t)ws.n_w * sizeof(sp_window_support), hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
}

int32_t sp_pileup_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_aln* aln,
                        const uint32_t* cigar, uint32_t cigar_stride, const uint32_t* n_cigar, const uint64_t* col_offset, sp_pileup_col* out) {
    if (!ctx) return SP_ERR_INVALID_ARG;
    if (!A || !B || !col_offset || (n_pairs && (!pairs || !aln || !n_cigar))) return sp_fail(ctx, SP_ERR_INVALID_ARG, "pileup: null argument");
    if (n_pairs > 0xFFFFFFFFull) return sp_fail(ctx, SP_ERR_INVALID_ARG, "pileup: too many pairs");
    int32_t rc = check_col_offset(ctx, "pileup", B, col_offset);
    if (rc != SP_OK) return rc;
    const uint64_t n_cols = col_offset[B->n];
    if (n_cols && !out) return sp_fail(ctx, SP_ERR_INVALID_ARG, "pileup: null argument");
    uint64_t total_ops = 0, n_ins_ops = 0;
    rc = pileup_check_rows(ctx, A, B, pairs, n_pairs, aln, cigar, cigar_stride, n_cigar, &total_ops, &n_ins_ops);
    if (rc != SP_OK) return rc;
    if (n_cols == 0) return SP_OK;
    const uint32_t n_t = B->n;
    uint64_t n_tiles = 0;
    rc = pu_count_tiles(ctx, "pileup", B, &n_tiles);
    if (rc != SP_OK) return rc;
    std::vector<uint32_t> bucket_off((size_t)n_t + 1, 0);                                 // the live pairs (those with ops) by target
    for (uint64_t i = 0; i < n_pairs; ++i) if (n_cigar[i]) ++bucket_off[pairs[i].b + 1];
    for (uint32_t t = 0; t < n_t; ++t) bucket_off[t + 1] += bucket_off[t];
    const uint32_t n_live = bucket_off[n_t];
    (void)hipSetDevice(ctx->device);
    // ---- one staging block, one copy: pairs in bucket order, bucket offsets, tiles, column offsets, the ops back to back
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t at_pairs = 0, at_bucket = up16(at_pairs + sizeof(PuPair) * (size_t)n_live), at_tiles = up16(at_bucket + 4 * ((size_t)n_t + 1)),
                 at_cols = up16(at_tiles + sizeof(PuTile) * (size_t)n_tiles), at_ops = up16(at_cols + 8 * ((size_t)n_t + 1)), in_bytes = up16(at_ops + 4 * (size_t)total_ops) + 16;
    uint8_t* h_in = (uint8_t*)sp_host_pool(ctx, "pileup_buckets", in_bytes);
    uint8_t* d_in = (uint8_t*)sp_pool(ctx, "pileup_buckets", in_bytes);
    uint32_t* d_out = (uint32_t*)sp_pool(ctx, "pileup_out", n_cols * sizeof(sp_pileup_col));
    if (!h_in || !d_in || !d_out) return sp_fail(ctx, SP_ERR_OUT_OF_MEMORY, "pileup buffers");
    {
        PuPair* hp = (PuPair*)(h_in + at_pairs); uint32_t* hops = (uint32_t*)(h_in + at_ops);
        std::vector<uint32_t> at(bucket_off.begin(), bucket_off.end() - 1);
        uint64_t op_at = 0;
        for (uint64_t i = 0; i < n_pairs; ++i) {
            if (n_cigar[i] == 0) continue;
            hp[at[pairs[i].b]++] = PuPair{ op_at, pairs[i].a, n_cigar[i], aln[i].b_start, aln[i].a_start };
            std::memcpy(hops + op_at, cigar + i * (size_t)cigar_stride, 4 * (size_t)n_cigar[i]);
            op_at += n_cigar[i];
        }
        std::memcpy(h_in + at_bucket, bucket_off.data(), 4 * ((size_t)n_t + 1));
        std::memcpy(h_in + at_cols, col_offset, 8 * ((size_t)n_t + 1));
        pu_fill_tiles(B, (PuTile*)(h_in + at_tiles));
    }
    SP_HIP_CHECK(ctx, hipMemcpyAsync(d_in, h_in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    rc = pileup_lds(ctx);
    if (rc != SP_OK) return rc;
    {
        ProfScope ps(ctx, "pileup", n_cols);
        hipLaunchKernelGGL(pileup_kernel, dim3((unsigned)n_tiles), dim3(PU_WAVES * SP_WAVE), PU_LDS_BYTES, ctx->stream, A->view(), B->d_len, (const PuPair*)(d_in + at_pairs),
                           (const uint32_t*)(d_in + at_bucket), (const uint32_t*)(d_in + at_ops), (const PuTile*)(d_in + at_tiles), (const uint64_t*)(d_in + at_cols), d_out);
        if (hipGetLastError() != hipSuccess) return sp_fail(ctx, SP_ERR_HIP, "pileup launch failed");
    }
    SP_HIP_CHECK(ctx, hipMemcpyAsync(out, d_out, n_cols * sizeof(sp_pileup_col), hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
}

int32_t sp_pileup_ins_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_aln* aln,
                            const uint32_t* cigar, uint32_t cigar_stride, const uint32_t* n_cigar, const uint64_t* col_offset, sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins) {
    if (!ctx) return SP_ERR_INVALID_ARG;
    if (!A || !B || !col_offset || !n_ins || (ins_cap && !ins) || (n_pairs && (!pairs || !aln || !n_cigar))) return sp_fail(ctx, SP_ERR_INVALID_ARG, "pileup: null argument");
    if (n_pairs > 0x7FFFFFFFull) return sp_fail(ctx, SP_ERR_INVALID_ARG, "pileup: too many pairs");
    int32_t rc = check_col_offset(ctx, "pileup", B, col_offset);
    if (rc != SP_OK) return rc;
    uint64_t total_ops = 0, n_ins_ops = 0;
    rc = pileup_check_rows(ctx, A, B, pairs, n_pairs, aln, cigar, cigar_stride, n_cigar, &total_ops, &n_ins_ops);
    if (rc != SP_OK) return rc;
    *n_ins = 0;
    if (n_ins_ops == 0 || col_offset[B->n] == 0) return SP_OK;
    HostRows hr;
    rc = stage_rows(ctx, B, pairs, (uint32_t)n_pairs, aln, cigar, cigar_stride, n_cigar, col_offset, total_ops, false, &hr);
    if (rc != SP_OK) return rc;
    InsPass ip;
    rc = ins_begin(ctx, "pileup", B, n_pairs, n_ins_ops, &ip);                            // (the host has counted the runs: the buffer is never too small)
    if (rc != SP_OK) return rc;
    rc = ins_collect(ctx, "pileup", ip, A, B, hr.pairs, hr.aln, hr.nc, hr.off, hr.ops, (uint32_t)n_pairs, 0, hr.cols);
    if (rc != SP_OK) return rc;
    uint64_t grow = 0;
    rc = ins_finish(ctx, "pileup", ip, ins, ins_cap, n_ins, &grow);
    if (rc != SP_OK) return rc;
    if (grow) return sp_fail(ctx, SP_ERR_HIP, "pileup: the run buffer did not hold the runs the host counted");
    return SP_OK;
}

int32_t sp_pileup_hap_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_aln* aln,
                            const uint32_t* cigar, uint32_t cigar_stride, const uint32_t* n_cigar, const uint64_t* col_offset,
                            sp_support_hap* haps, uint64_t hap_cap, uint64_t* n_haps, sp_support_hap_head* heads) {
    if (!ctx) return SP_ERR_INVALID_ARG;
    if (!A || !B || !col_offset || !n_haps || !heads || (hap_cap && !haps) || (n_pairs && (!pairs || !aln || !n_cigar))) return sp_fail(ctx, SP_ERR_INVALID_ARG, "pileup: null argument");
    if (n_pairs > 0x7FFFFFFFull) return sp_fail(ctx, SP_ERR_INVALID_ARG, "pileup: too many pairs");
    int32_t rc = check_col_offset(ctx, "pileup", B, col_offset);
    if (rc != SP_OK) return rc;
    uint64_t total_ops = 0, n_ins_ops = 0;
    rc = pileup_check_rows(ctx, A, B, pairs, n_pairs, aln, cigar, cigar_stride, n_cigar, &total_ops, &n_ins_ops);
    if (rc != SP_OK) return rc;
    *n_haps = 0;
    if (B->n == 0) return SP_OK;
    HostRows hr;
    rc = stage_rows(ctx, B, pairs, (uint32_t)n_pairs, aln, cigar, cigar_stride, n_cigar, col_offset, total_ops, true, &hr);
    if (rc == SP_OK && hr.n_tiles) rc = pileup_lds(ctx);
    if (rc != SP_OK) return rc;
    if (hr.n_tiles) {
        ProfScope ps(ctx, "pileup", col_offset[B->n]);
        hipLaunchKernelGGL(pileup_rows_kernel, dim3((unsigned)hr.n_tiles), dim3(PU_WAVES * SP_WAVE), PU_LDS_BYTES, ctx->stream, A->view(), B->d_len, hr.pairs, hr.aln, hr.nc, hr.off, hr.ops,
                           hr.order, hr.boff, 1u, 0u, hr.tiles, hr.cols, hr.table);
        if (hipGetLastError() != hipSuccess) return sp_fail(ctx, SP_ERR_HIP, "pileup launch failed");
    }
    HapOut ho; ho.haps = haps; ho.cap = hap_cap; ho.n_haps = n_haps; ho.heads = heads;
    return hap_run(ctx, "pileup", A, B, (uint32_t)n_pairs, hr.table, hr.cols, hr.pairs, hr.aln, hr.nc, hr.off, hr.ops, hr.order, hr.boff, 1, ho);
}

} // extern "C"

// sp_align_pileup_hap_batch for the library's own callers as well (sp_support.hip; declared in sp_internal.h): `who` begins its error texts, prof[] names its four launches (map, second map, pileup, summary) in the
// context's profile, and the first map launch counts the pairs it attempts (max_ed >= 0) when count_attempted is set, every pair of the slice otherwise.
int32_t align_pileup_run(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_opts* opts, int32_t band, int32_t retry_band,
                         const uint64_t* col_offset, sp_affine_aln* aln, sp_pileup_col* cols, sp_support_summary* summaries, const uint32_t* n_members, uint32_t* band_used,
                         const std::string& who, const char* const prof[4], bool count_attempted, sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins, uint64_t ins_runs, const HapOut* hap,
                         const WinIn* win) {
    if (!A || !B || !opts || !col_offset || (n_pairs && !pairs) || (ins && !n_ins) || (hap && (!hap->n_haps || !hap->heads))) return sp_fail(ctx, SP_ERR_INVALID_ARG, who + ": null argument");
    if ((band != 64 && band != 256) || (retry_band != 0 && retry_band != 256) || (retry_band != 0 && band != 64))
        return sp_fail(ctx, SP_ERR_INVALID_ARG, who + ": band must be 64 or 256, retry_band 0 or (with band 64) 256");
    if (n_pairs > 0x7FFFFFFFull) return sp_fail(ctx, SP_ERR_INVALID_ARG, who + ": too many pairs");
    const uint32_t n_t = B->n, n = (uint32_t)n_pairs;
    const int32_t rc_cols = check_col_offset(ctx, who, B, col_offset);
    if (rc_cols != SP_OK) return rc_cols;
    const uint64_t n_cols = col_offset[n_t];
    // ---- the pairs by target, from `pairs` alone: target t's pairs of slice s are order[boff[t * (n_slices + 1) + s] ...) (pileup_rows_kernel)
    const uint32_t n_slices = std::max<uint32_t>(1, (n + SP_ALIGN_PILEUP_SLICE - 1) / SP_ALIGN_PILEUP_SLICE);
    std::vector<uint32_t> boff((size_t)n_t * (n_slices + 1) + 1, 0);
    for (uint32_t i = 0; i < n; ++i) {
        if (pairs[i].a >= A->n || pairs[i].b >= B->n) return sp_fail(ctx, SP_ERR_INVALID_ARG, who + ": index out of range");
        ++boff[(size_t)pairs[i].b * (n_slices + 1) + i / SP_ALIGN_PILEUP_SLICE + 1];
    }
    if (win && !win->windows) win = nullptr;                                                          // (no windows: the call without them)
    WinStage ws;                                                                                      // the windows are checked before anything is launched or written
    if (win) { const int32_t rc = win_plan(ctx, who, B, win, 0, &ws); if (rc != SP_OK) return rc; if (ws.n_w == 0) win = nullptr; }
    if (ins) *n_ins = 0;
    if (hap) *hap->n_haps = 0;
    if (n_pairs == 0 && n_t == 0) return SP_OK;
    const bool want_table = (cols || summaries || hap) && n_t > 0;                                    // (the haplotype list reads the finished table)
    if (!aln && !want_table && !ins && !win) return SP_OK;
    // boff[t * (S + 1) + s + 1] holds the count of (t, s): into running offsets; entry t * (S + 1) is where target t begins = where target t - 1 ended
    {
        uint32_t run = 0;
        for (uint32_t t = 0; t < n_t; ++t) {
            uint32_t* row = boff.data() + (size_t)t * (n_slices + 1);
            row[0] = run;
            for (uint32_t s2 = 0; s2 < n_slices; ++s2) { run += row[s2 + 1]; row[s2 + 1] = run; }
        }
    }
    uint64_t n_tiles = 0;
    const int32_t rc_tiles = want_table ? pu_count_tiles(ctx, who, B, &n_tiles) : SP_OK;
    if (rc_tiles != SP_OK) return rc_tiles;
    (void)hipSetDevice(ctx->device);
    // ---- one staging block, one copy: the pair list as given, the order, the offsets, tiles, column offsets, member counts
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t at_pairs = 0, at_order = up16(at_pairs + sizeof(sp_pair) * (size_t)n), at_boff = up16(at_order + 4 * (size_t)n), at_tiles = up16(at_boff + 4 * boff.size()),
                 at_cols = up16(at_tiles + sizeof(PuTile) * (size_t)n_tiles), at_mem = up16(at_cols + 8 * ((size_t)n_t + 1));
    if (win) { const int32_t rc = win_plan(ctx, who, B, win, up16(at_mem + 4 * (size_t)n_t), &ws); if (rc != SP_OK) return rc; }      // (the windows' part behind the member counts)
    const size_t in_bytes = (win ? ws.end : up16(at_mem + 4 * (size_t)n_t)) + 16;
    uint8_t* h_in = (uint8_t*)sp_host_pool(ctx, "appile_in", in_bytes);
    uint64_t* h_st = (uint64_t*)sp_host_pool(ctx, "appile_st", 16);
    uint8_t* d_in = (uint8_t*)sp_pool(ctx, "appile_in", in_bytes);
    sp_affine_aln* d_aln = (sp_affine_aln*)sp_pool(ctx, "appile_aln", std::max<size_t>(16, (size_t)n * sizeof(sp_affine_aln)));
    uint32_t* d_nc = (uint32_t*)sp_pool(ctx, "appile_nc", std::max<size_t>(16, (size_t)n * 4));
    uint64_t* d_off = (uint64_t*)sp_pool(ctx, "appile_off", (size_t)n * 8 + 32);                   // (+ the cursor, the two status words and the retry list's counter)
    const uint32_t slice_max = std::min<uint32_t>(std::max<uint32_t>(n, 1), SP_ALIGN_PILEUP_SLICE);
    uint32_t* d_retry = retry_band ? (uint32_t*)sp_pool(ctx, "appile_retry", (size_t)slice_max * 8) : nullptr;      // the list as the waves made it, and in pair order
    uint32_t* d_band = (retry_band || band_used) ? (uint32_t*)sp_pool(ctx, "appile_band", std::max<size_t>(16, (size_t)n * 4)) : nullptr;
    uint32_t* d_table = want_table ? (uint32_t*)sp_pool(ctx, "appile_out", std::max<size_t>(16, n_cols * sizeof(sp_pileup_col))) : nullptr;
    sp_support_summary* d_sum = summaries && n_t ? (sp_support_summary*)sp_pool(ctx, "appile_sum", (size_t)n_t * sizeof(sp_support_summary)) : nullptr;
    sp_window_support* d_win = win ? (sp_window_support*)sp_pool(ctx, "appile_win", (size_t)ws.n_w * sizeof(sp_window_support)) : nullptr;
    if (win && !d_win) return sp_fail(ctx, SP_ERR_OUT_OF_MEMORY, who + " buffers");
    if (!h_in || !h_st || !d_in || !d_aln || !d_nc || !d_off || (retry_band && !d_retry) || ((retry_band || band_used) && !d_band) || (want_table && !d_table) || (summaries && n_t && !d_sum)) return sp_fail(ctx, SP_ERR_OUT_OF_MEMORY, who + " buffers");
    unsigned long long* d_cur = (unsigned long long*)(d_off + n); uint32_t* d_status = (uint32_t*)(d_off + n + 1); uint32_t* d_n_retry = (uint32_t*)(d_off + n + 2);
    {
        if (n) std::memcpy(h_in + at_pairs, pairs, sizeof(sp_pair) * (size_t)n);
        uint32_t* ho = (uint32_t*)(h_in + at_order);
        std::vector<uint32_t> at(n_t);
        for (uint32_t t = 0; t < n_t; ++t) at[t] = boff[(size_t)t * (n_slices + 1)];
        for (uint32_t i = 0; i < n; ++i) ho[at[pairs[i].b]++] = i;                                 // (by target, then in the order given: a slice's pairs of a target are consecutive)
        std::memcpy(h_in + at_boff, boff.data(), 4 * boff.size());
        std::memcpy(h_in + at_cols, col_offset, 8 * ((size_t)n_t + 1));
        if (n_members && n_t) std::memcpy(h_in + at_mem, n_members, 4 * (size_t)n_t);
        if (want_table) pu_fill_tiles(B, (PuTile*)(h_in + at_tiles));
        if (win) win_fill(ws, h_in, B, win);
    }
    SP_HIP_CHECK(ctx, hipMemcpyAsync(d_in, h_in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    const sp_pair* d_pairs = (const sp_pair*)(d_in + at_pairs);
    const uint32_t* d_order = (const uint32_t*)(d_in + at_order); const uint32_t* d_boff = (const uint32_t*)(d_in + at_boff);
    if (n_tiles) {
        const int32_t rc = pileup_lds(ctx);
        if (rc != SP_OK) return rc;
    }
    InsPass ip;                                                                                       // the insertion list, when asked for: its runs are collected slice by slice
    if (ins) {
        // the first guess: one run per 64 query bases (HiFi members against their own consensus carry far fewer) on top of four per pair; more than that runs the pass again
        uint64_t q_bases = 0;
        for (uint32_t i = 0; i < n; ++i) q_bases += (uint64_t)A->h_len[pairs[i].a];
        const int32_t rc = ins_begin(ctx, who, B, n_pairs, ins_runs ? ins_runs : 1024 + 4 * n_pairs + q_bases / 64, &ip);
        if (rc != SP_OK) return rc;
    }
    // ---- slice by slice: the map into the op buffer (run again on a larger one when it asked for more: a warm context does not), what the host must know, the pileup
    // With the haplotype list the buffer holds the rows of the WHOLE batch (the contested columns are known only behind the last slice): the cursor is not rewound
    // between slices.  A buffer that turns out too small behind the first slice must not lose the rows it holds: the batch moves into the context's second op buffer
    // ("appile_ops_b": the rows so far are copied, the slice runs again), sized from what the slices so far took per pair; nothing else is run again.  A warm context
    // begins on the larger of the two.  Without the list only "appile_ops" is used, as before.
    const bool keep_rows = hap && n_slices > 1;
    const char* ops_name = (keep_rows && sp_pool_bytes(ctx, "appile_ops_b") > sp_pool_bytes(ctx, "appile_ops")) ? "appile_ops_b" : "appile_ops";
    uint64_t ops_cap = std::max<uint64_t>(sp_pool_bytes(ctx, ops_name) / 4, (uint64_t)std::min<uint32_t>(std::max<uint32_t>(n, 1), keep_rows ? n : SP_ALIGN_PILEUP_SLICE) * 64);
    uint64_t kept = 0;                                                                                // (keep_rows) the cursor behind the last finished slice
    uint64_t* h_keep = keep_rows ? (uint64_t*)sp_host_pool(ctx, "appile_keep", 16) : nullptr;
    if (keep_rows && !h_keep) return sp_fail(ctx, SP_ERR_OUT_OF_MEMORY, who + " buffers");
    uint32_t* d_ops = nullptr;
    for (uint32_t s2 = 0; s2 < n_slices; ++s2) {
        const uint32_t p0 = s2 * SP_ALIGN_PILEUP_SLICE, m = std::min<uint32_t>(SP_ALIGN_PILEUP_SLICE, n - p0);
        for (int attempt = 0; m > 0; ++attempt) {
            d_ops = (uint32_t*)sp_pool(ctx, ops_name, (size_t)ops_cap * 4);
            if (!d_ops) return sp_fail(ctx, SP_ERR_OUT_OF_MEMORY, who + ": op rows");
            if (keep_rows && s2 > 0) {
                SP_HIP_CHECK(ctx, hipMemsetAsync(d_cur + 1, 0, 24, ctx->stream));                        // (the status words and the retry counter; the cursor stands ...
                if (attempt > 0) { *h_keep = kept; SP_HIP_CHECK(ctx, hipMemcpyAsync(d_cur, h_keep, 8, hipMemcpyHostToDevice, ctx->stream)); }      // ... or goes back behind the last finished slice)
            } else SP_HIP_CHECK(ctx, hipMemsetAsync(d_cur, 0, 32, ctx->stream));
            uint64_t attempted = m;
            if (count_attempted) { attempted = 0; for (uint32_t i = 0; i < m; ++i) attempted += pairs[p0 + i].max_ed >= 0 ? 1 : 0; }
            int rc = sp_launch_affine_map(ctx, A, B, d_pairs + p0, m, *opts, band, d_aln + p0, d_nc + p0, d_off + p0, d_ops, ops_cap, d_cur, prof[0], nullptr, nullptr, attempted);
            if (rc != SP_OK) return rc;
            if (retry_band) {
                // the second try: the list, in pair order, then the map on retry_band over it -- its length read from device memory, its results in place, its ops behind the first launch's
                hipLaunchKernelGGL(ap_retry_list_kernel, dim3((m + 255) / 256), dim3(256), 0, ctx->stream, d_pairs + p0, d_aln + p0, d_nc + p0, m, d_retry, d_n_retry, d_band + p0);
                hipLaunchKernelGGL(ap_retry_sort_kernel, dim3((m + 255) / 256), dim3(256), 0, ctx->stream, d_retry, d_n_retry, d_retry + slice_max);
                if (hipGetLastError() != hipSuccess) return sp_fail(ctx, SP_ERR_HIP, who + ": retry list launch failed");
                rc = sp_launch_affine_map(ctx, A, B, d_pairs + p0, m, *opts, retry_band, d_aln + p0, d_nc + p0, d_off + p0, d_ops, ops_cap, d_cur, prof[1], d_n_retry, d_retry + slice_max, 0);
                if (rc != SP_OK) return rc;
            }
            hipLaunchKernelGGL(ap_status_kernel, dim3((m + 255) / 256), dim3(256), 0, ctx->stream, d_aln + p0, d_nc + p0, d_off + p0, m, d_status);
            SP_HIP_CHECK(ctx, hipMemcpyAsync(h_st, d_cur, 16, hipMemcpyDeviceToHost, ctx->stream));
            if (hipStreamSynchronize(ctx->stream) != hipSuccess) return sp_fail(ctx, SP_ERR_HIP, who + ": the map kernel failed");
            if (h_st[0] <= ops_cap) break;
            if (attempt == 1) return sp_fail(ctx, SP_ERR_HIP, who + ": the op buffer did not hold a second run");
            if (keep_rows && s2 > 0) {
                // what this slice needs on top of the rows kept, and for the pairs still to come what the pairs so far took each, and a quarter
                const uint64_t done = (uint64_t)p0 + m, per_pair = (h_st[0] + done - 1) / done;
                const uint64_t new_cap = std::max<uint64_t>(2 * ops_cap, h_st[0] + per_pair * (n - done) * 5 / 4 + 64);
                const char* other = std::strcmp(ops_name, "appile_ops") == 0 ? "appile_ops_b" : "appile_ops";
                uint32_t* d_new = (uint32_t*)sp_pool(ctx, other, (size_t)new_cap * 4);
                if (!d_new) return sp_fail(ctx, SP_ERR_OUT_OF_MEMORY, who + ": op rows");
                if (kept) SP_HIP_CHECK(ctx, hipMemcpyAsync(d_new, d_ops, (size_t)kept * 4, hipMemcpyDeviceToDevice, ctx->stream));
                ops_name = other; ops_cap = new_cap;
                continue;
            }
            ops_cap = h_st[0];
        }
        if (keep_rows && m > 0) kept = h_st[0];
        if (m > 0) {
            const uint32_t* st = (const uint32_t*)(h_st + 1);
            if (st[0]) return sp_fail(ctx, SP_ERR_HIP, who + ": a walk did not reach the cell its path started in");
            if (st[1]) return sp_fail(ctx, SP_ERR_CAPACITY, who + ": an alignment of more than 4,096 runs");
        }
        if (n_tiles) {
            ProfScope ps(ctx, prof[2], n_cols);
            hipLaunchKernelGGL(pileup_rows_kernel, dim3((unsigned)n_tiles), dim3(PU_WAVES * SP_WAVE), PU_LDS_BYTES, ctx->stream, A->view(), B->d_len, d_pairs, d_aln, d_nc, d_off, d_ops,
                               d_order, d_boff, n_slices, s2, (const PuTile*)(d_in + at_tiles), (const uint64_t*)(d_in + at_cols), d_table);
            if (hipGetLastError() != hipSuccess) return sp_fail(ctx, SP_ERR_HIP, who + ": pileup launch failed");
        }
        if (win) {
            const int32_t rc = win_launch(ctx, who, ws, d_in, d_aln, d_nc, d_off, d_ops, d_order, d_boff, n_slices, s2, d_win);
            if (rc != SP_OK) return rc;
        }
        if (ins && m > 0) {
            const int32_t rc = ins_collect(ctx, who, ip, A, B, d_pairs + p0, d_aln + p0, d_nc + p0, d_off + p0, d_ops, m, p0, (const uint64_t*)(d_in + at_cols));
            if (rc != SP_OK) return rc;
        }
    }
    if (d_sum) {
        ProfScope ps(ctx, prof[3], n_cols);
        hipLaunchKernelGGL(support_summary_kernel, dim3(n_t), dim3(AP_SUM_THREADS), 0, ctx->stream, d_table, (const uint64_t*)(d_in + at_cols), B->d_len, d_aln, d_order, d_boff, n_slices,
                           n_members ? (const uint32_t*)(d_in + at_mem) : nullptr, d_sum);
        if (hipGetLastError() != hipSuccess) return sp_fail(ctx, SP_ERR_HIP, who + ": summary launch failed");
    }
    if (band_used && n) {
        hipLaunchKernelGGL(ap_band_used_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_aln, d_nc, n, (uint32_t)band, (uint32_t)retry_band, retry_band ? 1 : 0, d_band);
        if (hipGetLastError() != hipSuccess) return sp_fail(ctx, SP_ERR_HIP, who + ": band_used launch failed");
    }
    // ---- only what was asked for comes back
    if (band_used && n) SP_HIP_CHECK(ctx, hipMemcpyAsync(band_used, d_band, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (aln && n) SP_HIP_CHECK(ctx, hipMemcpyAsync(aln, d_aln, (size_t)n * sizeof(sp_affine_aln), hipMemcpyDeviceToHost, ctx->stream));
    if (cols && n_cols) SP_HIP_CHECK(ctx, hipMemcpyAsync(cols, d_table, n_cols * sizeof(sp_pileup_col), hipMemcpyDeviceToHost, ctx->stream));
    if (d_sum) SP_HIP_CHECK(ctx, hipMemcpyAsync(summaries, d_sum, (size_t)n_t * sizeof(sp_support_summary), hipMemcpyDeviceToHost, ctx->stream));
    if (win) SP_HIP_CHECK(ctx, hipMemcpyAsync(win->out, d_win, (size_t)ws.n_w * sizeof(sp_window_support), hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    int32_t rc_ins = SP_OK;
    if (ins) {
        // the lists last: everything else is complete when one does not fit.  A run buffer that was guessed too small: the whole pass once more on one that holds them
        // (the op rows of the earlier slices are gone) -- a warm context's buffer is large enough.  That is decided before the haplotype list is made.
        uint64_t grow = 0;
        rc_ins = ins_finish(ctx, who, ip, ins, ins_cap, n_ins, &grow);
        if (rc_ins != SP_OK && !(hap && rc_ins == SP_ERR_CAPACITY && *n_ins > ins_cap)) return rc_ins;      // (with the other list asked for, that one is still made)
        if (grow) {
            if (ins_runs) return sp_fail(ctx, SP_ERR_HIP, who + ": the run buffer did not hold a second run");
            return align_pileup_run(ctx, A, B, pairs, n_pairs, opts, band, retry_band, col_offset, aln, cols, summaries, n_members, band_used, who, prof, count_attempted, ins, ins_cap, n_ins, grow, hap, win);
        }
    }
    if (hap) {
        const int32_t rc = hap_run(ctx, who, A, B, n, d_table, (const uint64_t*)(d_in + at_cols), d_pairs, d_aln, d_nc, d_off, d_ops, d_order, d_boff, n_slices, *hap);
        if (rc != SP_OK) return rc;
    }
    if (rc_ins != SP_OK) return sp_fail(ctx, rc_ins, who + ": " + std::to_string(*n_ins) + " insertion records, room for " + std::to_string(ins_cap));
    return SP_OK;
}

extern "C" {

static const char* const AP_PROF[4] = { "align_pileup_map", "align_pileup_map_retry", "align_pileup_pile", "align_pileup_summary" };

// sp_align_pileup_band_batch with windows: the same path, no list
int32_t sp_align_pileup_windows_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_opts* opts, int32_t band, int32_t retry_band,
                                      const uint64_t* col_offset, sp_affine_aln* aln, sp_pileup_col* cols, sp_support_summary* summaries, const uint32_t* n_members, uint32_t* band_used,
                                      const uint64_t* win_offset, const sp_window* windows, sp_window_support* win_out) {
    if (!ctx) return SP_ERR_INVALID_ARG;
    if (windows && !win_offset) return sp_fail(ctx, SP_ERR_INVALID_ARG, "align_pileup: null argument");
    const WinIn win = { win_offset, windows, win_out };
    return align_pileup_run(ctx, A, B, pairs, n_pairs, opts, band, retry_band, col_offset, aln, cols, summaries, n_members, band_used, "align_pileup", AP_PROF, false, nullptr, 0, nullptr, 0,
                            nullptr, windows ? &win : nullptr);
}

int32_t sp_align_pileup_hap_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_opts* opts, int32_t band, int32_t retry_band,
                                  const uint64_t* col_offset, sp_affine_aln* aln, sp_pileup_col* cols, sp_support_summary* summaries, const uint32_t* n_members, uint32_t* band_used,
                                  sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins, sp_support_hap* haps, uint64_t hap_cap, uint64_t* n_haps, sp_support_hap_head* heads) {
    if (!ctx) return SP_ERR_INVALID_ARG;
    const char* const* prof = AP_PROF;
    HapOut ho; ho.haps = haps; ho.cap = hap_cap; ho.n_haps = n_haps; ho.heads = heads;
    return align_pileup_run(ctx, A, B, pairs, n_pairs, opts, band, retry_band, col_offset, aln, cols, summaries, n_members, band_used, "align_pileup", prof, false, ins, ins_cap, n_ins, 0,
                            haps ? &ho : nullptr, nullptr);
}

// the entries without one list or both: the same path, the list's arguments NULL
int32_t sp_align_pileup_ins_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_opts* opts, int32_t band, int32_t retry_band,
                                  const uint64_t* col_offset, sp_affine_aln* aln, sp_pileup_col* cols, sp_support_summary* summaries, const uint32_t* n_members, uint32_t* band_used,
                                  sp_pileup_ins* ins, uint64_t ins_cap, uint64_t* n_ins) {
    return sp_align_pileup_hap_batch(ctx, A, B, pairs, n_pairs, opts, band, retry_band, col_offset, aln, cols, summaries, n_members, band_used, ins, ins_cap, n_ins, nullptr, 0, nullptr, nullptr);
}

int32_t sp_align_pileup_band_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_opts* opts, int32_t band, int32_t retry_band,
                                   const uint64_t* col_offset, sp_affine_aln* aln, sp_pileup_col* cols, sp_support_summary* summaries, const uint32_t* n_members, uint32_t* band_used) {
    return sp_align_pileup_ins_batch(ctx, A, B, pairs, n_pairs, opts, band, retry_band, col_offset, aln, cols, summaries, n_members, band_used, nullptr, 0, nullptr);
}

int32_t sp_align_pileup_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_opts* opts, const uint64_t* col_offset,
                              sp_affine_aln* aln, sp_pileup_col* cols, sp_support_summary* summaries, const uint32_t* n_members) {
    return sp_align_pileup_band_batch(ctx, A, B, pairs, n_pairs, opts, 64, 0, col_offset, aln, cols, summaries, n_members, nullptr);
}

} // extern "C"

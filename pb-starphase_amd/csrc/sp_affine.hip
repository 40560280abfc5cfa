// sp_affine.hip -- the two-piece affine re-score of an alignment the library found: the numbers the reference reports.
//
// Every (nm, start, end) of the reference is minimap2's (`standard_hifi_aligner`, src/util/mapping.rs:8-14: map-hifi, match 1 -- 5 in score_read,
// src/hla/caller.rs:1370-1379 --, mismatch 4, gaps min(6 + 2 l, 26 + l), ambiguous bases -1): an alignment through the chain's seeds, global between
// them and extended from the outermost ones to the best-scoring cell, i.e. the best LOCAL alignment through its seeds.  The library's own cell (anchor +
// unit-cost wavefront, sp_wfa.hip.h) decides which pairs align and on which diagonal; this kernel then re-scores a pair the reference's way: the banded
// Smith-Waterman optimum under those scores on the 64 or 256 diagonals around the cell's diagonal, with the forward decisions and end rules of
// oracle/affine.c (the CPU statement this kernel is bit-exact against; oracle/mm2.c is the minimap2 restatement it is measured against:
// tests/test_oracle_affine.py -- identical (nm, spans) on every audited K1 / K2 pair, 98.7 % of the K3 hits inside the 5 % filter).
//
// One wavefront per pair, lane l holds DPL consecutive diagonals (1: 64 diagonals, 4: 256), one target row per step.  Per cell three states come from the
// row before (H on the same diagonal, H / E / E2 on the next one: one DPP move each) and the two insertion states run ALONG the row: F(j) = max over
// j' < j of H(j') - q - (j - j') e is a max-plus prefix scan over the lanes -- the gfx9 DPP scan (row_shr 1, 2, 4, 8, row_bcast 15 / 31) on a packed
// key (score + position * e, ties to the nearest opening, as the sequential recurrence decides them) with the path's counters riding along.  Every state
// carries the mismatch + gap + ambiguous bases of its path and the cell it began in: the result needs no traceback and no memory beyond the two packed
// sequences in LDS.  sp_affine_align_batch (affine_tb_kernel, below) is the same pass with a direction record per cell and the walk back through them: the path itself.
#include "sp_internal.h"
#include "sp_wfa.hip.h"
#include <mutex>
#include <set>
#include <string>

namespace {

constexpr int AF_NEG = -(1 << 28);
constexpr uint32_t AF_BIAS = 1u << 22;

struct AfState { int s; uint32_t m0, m1; };                 // score; start cell (i << 16 | j); mismatch + gap + ambiguous bases of the path
struct AfKey { uint32_t k, m0, m1; };                       // scan element: (score + pos * e + bias) << 8 | pos, and the counters of that cell's path

__device__ __forceinline__ AfState af_none() { AfState x; x.s = AF_NEG; x.m0 = 0; x.m1 = 0; return x; }
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ AfKey af_dpp(const AfKey& v) {
    AfKey r;
    r.k = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.k, CTRL, ROW_MASK, 0xf, false);
    r.m0 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.m0, CTRL, ROW_MASK, 0xf, false);
    r.m1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.m1, CTRL, ROW_MASK, 0xf, false);
    return r;
}
__device__ __forceinline__ AfKey af_max(const AfKey& a, const AfKey& b) { return b.k > a.k ? b : a; }
// inclusive prefix maximum over the 64 lanes (keys are unique per position, 0 = nothing)
__device__ __forceinline__ AfKey af_scan(AfKey v) {
    v = af_max(v, af_dpp<0x111, 0xf>(v));                   // row_shr:1
    v = af_max(v, af_dpp<0x112, 0xf>(v));                   // row_shr:2
    v = af_max(v, af_dpp<0x114, 0xf>(v));                   // row_shr:4
    v = af_max(v, af_dpp<0x118, 0xf>(v));                   // row_shr:8
    v = af_max(v, af_dpp<0x142, 0xa>(v));                   // row_bcast:15 into rows 1 and 3
    v = af_max(v, af_dpp<0x143, 0xc>(v));                   // row_bcast:31 into rows 2 and 3
    return v;
}
__device__ __forceinline__ AfKey af_from_lower(const AfKey& v) {          // lane l - 1's value, nothing for lane 0
    AfKey r;
    r.k = (uint32_t)spw::from_lower((int)v.k, 0); r.m0 = (uint32_t)spw::from_lower((int)v.m0, 0); r.m1 = (uint32_t)spw::from_lower((int)v.m1, 0);
    return r;
}
__device__ __forceinline__ AfState af_from_upper(const AfState& v) {      // lane l + 1's value, nothing for lane 63
    AfState r;
    r.s = spw::from_upper(v.s, AF_NEG); r.m0 = (uint32_t)spw::from_upper((int)v.m0, 0); r.m1 = (uint32_t)spw::from_upper((int)v.m1, 0);
    return r;
}

struct AfPair { uint32_t a, b; int32_t diag, pad; };        // a = query (set A), b = target (set B), diag = b_pos - a_pos (the library's convention)
// The rows of a pair the DP has to run (sp_rescore_mappings, below): the stretches of the alignment whose edits do not stand alone.  r0 >= 0: the DP starts at target
// row r0 with ONE live cell in the row before it, diagonal index idx_in, holding the alignment's closed-form score up to there (s_in, nm_in, start_cell); r1 >= 0:
// when row r1 is done and the cell on diagonal idx_out is the one best cell of the row, the rest of the alignment is added in closed form (d_score, d_nm, its end
// end_t / end_q) and the DP stops; otherwise it runs on to the last row.  Between two stretches (n_mid of them, AfMid): when row r_exit is done and the cell on idx_out
// is the one best cell of the row, the DP goes on at row r_entry from that cell alone, d_score / d_nm later, on diagonal idx_in; otherwise it runs through.
struct AfWin { int32_t r0, idx_in, s_in, nm_in; uint32_t start_cell; int32_t r1, idx_out, d_score, d_nm, end_t, end_q, n_mid; };
struct AfMid { int32_t r_exit, idx_out, d_score, d_nm, r_entry, idx_in; };
constexpr int AF_MAXMID = 15;

template <int DPL, bool HASN>
__global__ __launch_bounds__(64) void affine_kernel(SeqSetView A, SeqSetView B, const AfPair* __restrict__ pairs, uint32_t n_pairs, const uint32_t* __restrict__ n_live, sp_affine_opts o,
                                                     sp_affine_aln* __restrict__ out, int t_words_max, const AfWin* __restrict__ wins, const AfMid* __restrict__ mids) {
    extern __shared__ uint32_t lds[];
    const uint32_t p = blockIdx.x;
    if (p >= n_pairs || (n_live && p >= *n_live)) return;              // (n_live: the number of pairs a kernel before this one left in the list)
    const int lane = threadIdx.x;
    const AfPair pr = pairs[p];
    const int tlen = B.len[pr.b], qlen = A.len[pr.a];
    sp_affine_aln res; res.score = 0; res.nm = 0; res.a_start = res.a_end = res.b_start = res.b_end = 0;
    constexpr int BAND = 64 * DPL;
    const int klo = -pr.diag - BAND / 2;                    // diagonal k = q_pos - t_pos of lane 0's first cell
    int i_lo = -(klo + BAND - 1); if (i_lo < 0) i_lo = 0;
    int i_hi = qlen - 1 - klo; if (i_hi > tlen - 1) i_hi = tlen - 1;
    if (pr.pad < 0 || tlen <= 0 || qlen <= 0 || i_lo > i_hi) { if (lane == 0) out[p] = res; return; }      // (a pair marked "skip" by the library's own callers: max_ed < 0)
    // the rows of the target and the query bases they can meet, packed as they are in memory (2 bits per base, + the N plane when the set has one)
    constexpr bool hasn = HASN;
    const int tw0 = i_lo >> 4, tw1 = (i_hi >> 4) + 1;                                   // target words [tw0, tw1)
    int q_lo = i_lo + klo; if (q_lo < 0) q_lo = 0;
    int q_hi = i_hi + klo + BAND - 1; if (q_hi > qlen - 1) q_hi = qlen - 1;
    const int qw0 = q_lo >> 4, qw1 = (q_hi >> 4) + 1;
    uint32_t* LT = lds; uint32_t* LQ = LT + t_words_max; uint32_t* NT = LQ + t_words_max + 2 * BAND / 16 + 8; uint32_t* NQ = NT + t_words_max;
    {
        const uint32_t* tw = B.words + B.word_off[pr.b]; const uint32_t* qw = A.words + A.word_off[pr.a];
        const uint32_t* tn = B.nplane ? B.nplane + B.word_off[pr.b] : nullptr; const uint32_t* qn = A.nplane ? A.nplane + A.word_off[pr.a] : nullptr;
        for (int w = lane; w < tw1 - tw0; w += SP_WAVE) { LT[w] = tw[tw0 + w]; if (hasn) NT[w] = tn ? tn[tw0 + w] : 0u; }
        for (int w = lane; w < qw1 - qw0; w += SP_WAVE) { LQ[w] = qw[qw0 + w]; if (hasn) NQ[w] = qn ? qn[qw0 + w] : 0u; }
    }
    spw::wave_lds_sync();
    auto base_of = [&](const uint32_t* W, const uint32_t* N, int pos, int w0) {
        const int w = (pos >> 4) - w0; const uint32_t sh = (uint32_t)(pos & 15) << 1;
        if (hasn && ((N[w] >> sh) & 1u)) return 4;
        return (int)((W[w] >> sh) & 3u);
    };
    AfState H[DPL], E1[DPL], E2[DPL];
#pragma unroll
    for (int c = 0; c < DPL; ++c) H[c] = E1[c] = E2[c] = af_none();
    int bs = 0, bi = -1, bj = -1; uint32_t bm0 = 0, bm1 = 0;
    const int q1 = o.q, e1 = o.e, q2 = o.q2, e2 = o.e2;
    AfWin win; win.r0 = -1; win.r1 = -1; win.n_mid = 0;
    if (wins) win = wins[p];
    int i_first = i_lo;
    if (win.r0 > i_lo && win.r0 <= i_hi && (unsigned)win.idx_in < (unsigned)BAND) {
        i_first = win.r0;
#pragma unroll
        for (int c = 0; c < DPL; ++c)
            if (lane * DPL + c == win.idx_in) {
                H[c].s = win.s_in; H[c].m0 = win.start_cell; H[c].m1 = (uint32_t)win.nm_in;
                bs = win.s_in; bi = win.r0 - 1; bj = win.r0 - 1 + klo + win.idx_in; bm0 = win.start_cell; bm1 = (uint32_t)win.nm_in;
            }
    }
    const int i_tail = (win.r1 >= i_first && win.r1 < i_hi && (unsigned)win.idx_out < (unsigned)BAND) ? win.r1 : -1;
    bool tail_ok = false; int tail_s = 0; uint32_t tail_m0 = 0, tail_m1 = 0;
    int mid_k = 0; AfMid mid; mid.r_exit = -1;
    if (win.n_mid > 0) mid = mids[(size_t)p * AF_MAXMID];
    int i_check = mid_k < win.n_mid ? mid.r_exit : i_tail, chk_idx = mid_k < win.n_mid ? mid.idx_out : win.idx_out;
    for (int i = i_first; i <= i_hi; ++i) {
        const int ct = base_of(LT, NT, i, tw0);
        // the diagonal above lane's last cell: lane l + 1's first cell of the row before
        const AfState upH = af_from_upper(H[0]), upE1 = af_from_upper(E1[0]), upE2 = af_from_upper(E2[0]);
        AfState hA[DPL], e1n[DPL], e2n[DPL]; AfKey k1[DPL], k2[DPL]; bool valid[DPL];
#pragma unroll
        for (int c = 0; c < DPL; ++c) {
            const int idx = lane * DPL + c, j = i + klo + idx;
            valid[c] = (unsigned)j < (unsigned)qlen;
            const AfState hu = c + 1 < DPL ? H[c + 1] : upH, eu = c + 1 < DPL ? E1[c + 1] : upE1, eu2 = c + 1 < DPL ? E2[c + 1] : upE2;
            AfState a1, a2;
            { const int eo = hu.s - q1; if (eu.s > eo) { a1 = eu; a1.s = eu.s - e1; } else { a1 = hu; a1.s = eo - e1; } a1.m1 += 1; }
            { const int eo = hu.s - q2; if (eu2.s > eo) { a2 = eu2; a2.s = eu2.s - e2; } else { a2 = hu; a2.s = eo - e2; } a2.m1 += 1; }
            if (a1.s < AF_NEG) a1.s = AF_NEG;
            if (a2.s < AF_NEG) a2.s = AF_NEG;
            AfState h = H[c];
            const int cq = valid[c] ? base_of(LQ, NQ, j, qw0) : 4;
            const bool ambi = ct > 3 || cq > 3;
            const int sub = ambi ? -o.sc_ambi : (ct == cq ? o.a : -o.b);
            if (h.s <= 0) { h.s = 0; h.m1 = 0; h.m0 = ((uint32_t)i << 16) | (uint32_t)(j & 0xFFFF); }
            h.s += sub; h.m1 += (ambi || ct != cq) ? 1u : 0u;
            if (a1.s > h.s) h = a1;                         // (F comes between E and E2 in the order of ties: below)
            if (!valid[c]) { h = af_none(); a1 = af_none(); a2 = af_none(); }
            hA[c] = h; e1n[c] = a1; e2n[c] = a2;
            // what this cell offers to the cells to its right as the opening of a gap: the best of its non-F states (an opening behind an F is never better
            // than that F continued), keyed so that the maximum over the cells to the left is the sequential recurrence's choice
            AfState src = h; if (a2.s > src.s) src = a2;
            if (src.s <= 0) { src.s = 0; }                 // (a cell nothing ends in: opening a gap from it scores below zero and never wins)
            const bool offer = valid[c] && src.s > 0;
            k1[c].k = offer ? (((uint32_t)(src.s + idx * e1) + AF_BIAS) << 8 | (uint32_t)idx) : 0u; k1[c].m0 = src.m0; k1[c].m1 = src.m1;
            k2[c].k = offer ? (((uint32_t)(src.s + idx * e2) + AF_BIAS) << 8 | (uint32_t)idx) : 0u; k2[c].m0 = src.m0; k2[c].m1 = src.m1;
        }
        // exclusive prefix maxima over the diagonals to the left: across the lanes by DPP, inside a lane cell by cell
        AfKey in1 = k1[0], in2 = k2[0];
#pragma unroll
        for (int c = 1; c < DPL; ++c) { in1 = af_max(in1, k1[c]); in2 = af_max(in2, k2[c]); }
        in1 = af_from_lower(af_scan(in1)); in2 = af_from_lower(af_scan(in2));
#pragma unroll
        for (int c = 0; c < DPL; ++c) {
            const int idx = lane * DPL + c, j = i + klo + idx;
            AfState f1 = af_none(), f2 = af_none();
            if (in1.k) { const int src_idx = (int)(in1.k & 0xFFu), v = (int)((in1.k >> 8) - AF_BIAS); f1.s = v - q1 - idx * e1; f1.m0 = in1.m0; f1.m1 = in1.m1 + (uint32_t)(idx - src_idx); }
            if (in2.k) { const int src_idx = (int)(in2.k & 0xFFu), v = (int)((in2.k >> 8) - AF_BIAS); f2.s = v - q2 - idx * e2; f2.m0 = in2.m0; f2.m1 = in2.m1 + (uint32_t)(idx - src_idx); }
            AfState h = hA[c];
            if (valid[c]) {
                if (f1.s > h.s) h = f1;
                if (e2n[c].s > h.s) h = e2n[c];
                if (f2.s > h.s) h = f2;
                if (h.s <= 0) { h.s = 0; h.m1 = 0; h.m0 = ((uint32_t)i << 16) | (uint32_t)(j & 0xFFFF); }
                const bool better = h.s > bs || (h.s == bs && h.s > 0 && (i + j < bi + bj || (i + j == bi + bj && i < bi)));
                bs = better ? h.s : bs; bi = better ? i : bi; bj = better ? j : bj; bm0 = better ? h.m0 : bm0; bm1 = better ? h.m1 : bm1;
            }
            H[c] = h; E1[c] = e1n[c]; E2[c] = e2n[c];
            in1 = af_max(in1, k1[c]); in2 = af_max(in2, k2[c]);
        }
        if (i == i_check) {
            // the row behind the last cluster: is the alignment where the library's own one runs, alone at the top of the row?
            int mine = AF_NEG, others = AF_NEG; uint32_t m0 = 0, m1 = 0;
#pragma unroll
            for (int c = 0; c < DPL; ++c) {
                if (lane * DPL + c == chk_idx) { mine = H[c].s; m0 = H[c].m0; m1 = H[c].m1; }
                else if (H[c].s > others) others = H[c].s;
            }
            const int src = chk_idx / DPL;
            const int s_exit = __shfl(mine, src);
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) { const int v = __shfl_xor(others, d); others = v > others ? v : others; }
            const bool alone = s_exit > 0 && others < s_exit;
            m0 = (uint32_t)__shfl((int)m0, src); m1 = (uint32_t)__shfl((int)m1, src);
            if (mid_k < win.n_mid) {
                if (alone && mid.r_entry > i && mid.r_entry <= i_hi && (unsigned)mid.idx_in < (unsigned)BAND) {
#pragma unroll
                    for (int c = 0; c < DPL; ++c) {
                        H[c] = E1[c] = E2[c] = af_none();
                        if (lane * DPL + c == mid.idx_in) {
                            const int s = s_exit + mid.d_score;
                            H[c].s = s; H[c].m0 = m0; H[c].m1 = m1 + (uint32_t)mid.d_nm;
                            if (s > bs) { bs = s; bi = mid.r_entry - 1; bj = mid.r_entry - 1 + klo + mid.idx_in; bm0 = m0; bm1 = H[c].m1; }
                        }
                    }
                    i = mid.r_entry - 1;
                }
                ++mid_k;
                if (mid_k < win.n_mid) mid = mids[(size_t)p * AF_MAXMID + mid_k];
                i_check = mid_k < win.n_mid ? mid.r_exit : i_tail; chk_idx = mid_k < win.n_mid ? mid.idx_out : win.idx_out;
            } else if (alone) {
                tail_ok = true; tail_s = s_exit + win.d_score; tail_m0 = m0; tail_m1 = m1 + (uint32_t)win.d_nm;
                break;
            } else i_check = -1;
        }
    }
    // the best cell of the wave: highest score, then the smallest anti-diagonal, then the smallest row
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const int os = __shfl_xor(bs, d), oi = __shfl_xor(bi, d), oj = __shfl_xor(bj, d);
        const uint32_t om0 = (uint32_t)__shfl_xor((int)bm0, d), om1 = (uint32_t)__shfl_xor((int)bm1, d);
        if (os > bs || (os == bs && os > 0 && (oi + oj < bi + bj || (oi + oj == bi + bj && oi < bi)))) { bs = os; bi = oi; bj = oj; bm0 = om0; bm1 = om1; }
    }
    if (tail_ok && tail_s > bs) { bs = tail_s; bi = win.end_t - 1; bj = win.end_q - 1; bm0 = tail_m0; bm1 = tail_m1; }      // (the end of the alignment lies behind every cell of the rows run: it wins only with the higher score)
    if (lane == 0) {
        if (bs > 0) { res.score = bs; res.nm = (int32_t)bm1; res.b_start = (int32_t)(bm0 >> 16); res.b_end = bi + 1; res.a_start = (int32_t)(bm0 & 0xFFFFu); res.a_end = bj + 1; }
        out[p] = res;
    }
}


// ------------------------------------------------------------------------------------------------------------------------------
// The same DP with its traceback (sp_affine_align_batch): HOW a pair aligns under the reference's scores.  The forward pass is affine_kernel's over all rows of the
// band (no AfWin / AfMid shortcuts), cell for cell, and additionally leaves ONE byte per cell in global memory, row by row:
//   bits 0-2  where H came from: the diagonal, E1, F1, E2, F2 (in the order of ties, each replacing only when strictly greater), the diagonal of a cell the path
//             STARTS in (the h.s <= 0 reset), or nothing (H = 0 / outside the rectangle)
//   bit 3 / 4 E1 / E2 of this cell continue the gap of the cell above (strictly better than opening one there)
//   bit 5 / 6 F1 / F2 of this cell continue the gap of the cell to the left (the scan key's source is not the nearest cell)
//   bit 7     the column of this cell is a mismatch or holds an ambiguous base
// The path is then not chosen afresh: from the forward pass's end cell the wave walks these records back to the cell the path started in.  The wave stages
// AF_TB_TILE bytes of direction rows into LDS at a time (over the packed sequences, which the walk does not need: bit 7) and lane 0 follows them, writing
// run-length ops backwards into the pair's own scratch behind its direction rows (a row adds at most two ops: a run of F steps and one step upwards); at the end
// they are copied out in forward order, the first `stride` of them.  Score, NM and spans are the forward pass's own.
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int AF_TB_TILE = 8192;
constexpr uint32_t AF_TB_LOST = 0xFFFFFFFFu;               // n_cigar of a pair whose walk did not arrive: the host turns it into an error
constexpr uint32_t AF_D_DIAG = 0, AF_D_E1 = 1, AF_D_F1 = 2, AF_D_E2 = 3, AF_D_F2 = 4, AF_D_START = 5, AF_D_NONE = 6;
constexpr uint32_t AF_D_E1C = 0x08, AF_D_E2C = 0x10, AF_D_F1C = 0x20, AF_D_F2C = 0x40, AF_D_X = 0x80;

template <int DPL, bool HASN>
__global__ __launch_bounds__(64) void affine_tb_kernel(SeqSetView A, SeqSetView B, const AfPair* __restrict__ pairs, uint32_t n_pairs, sp_affine_opts o, sp_affine_aln* __restrict__ out,
                                                        int t_words_max, uint8_t* __restrict__ scratch, const uint64_t* __restrict__ off, uint32_t* __restrict__ cigar, uint32_t stride,
                                                        uint32_t* __restrict__ n_cigar) {
    extern __shared__ uint32_t lds[];
    const uint32_t p = blockIdx.x;
    if (p >= n_pairs) return;
    const int lane = threadIdx.x;
    const AfPair pr = pairs[p];
    const int tlen = B.len[pr.b], qlen = A.len[pr.a];
    sp_affine_aln res; res.score = 0; res.nm = 0; res.a_start = res.a_end = res.b_start = res.b_end = 0;
    constexpr int BAND = 64 * DPL;
    const int klo = -pr.diag - BAND / 2;
    int i_lo = -(klo + BAND - 1); if (i_lo < 0) i_lo = 0;
    int i_hi = qlen - 1 - klo; if (i_hi > tlen - 1) i_hi = tlen - 1;
    if (pr.pad < 0 || tlen <= 0 || qlen <= 0 || i_lo > i_hi) { if (lane == 0) { out[p] = res; n_cigar[p] = 0; } return; }
    constexpr bool hasn = HASN;
    const int tw0 = i_lo >> 4, tw1 = (i_hi >> 4) + 1;
    int q_lo = i_lo + klo; if (q_lo < 0) q_lo = 0;
    int q_hi = i_hi + klo + BAND - 1; if (q_hi > qlen - 1) q_hi = qlen - 1;
    const int qw0 = q_lo >> 4, qw1 = (q_hi >> 4) + 1;
    uint32_t* LT = lds; uint32_t* LQ = LT + t_words_max; uint32_t* NT = LQ + t_words_max + 2 * BAND / 16 + 8; uint32_t* NQ = NT + t_words_max;
    {
        const uint32_t* tw = B.words + B.word_off[pr.b]; const uint32_t* qw = A.words + A.word_off[pr.a];
        const uint32_t* tn = B.nplane ? B.nplane + B.word_off[pr.b] : nullptr; const uint32_t* qn = A.nplane ? A.nplane + A.word_off[pr.a] : nullptr;
        for (int w = lane; w < tw1 - tw0; w += SP_WAVE) { LT[w] = tw[tw0 + w]; if (hasn) NT[w] = tn ? tn[tw0 + w] : 0u; }
        for (int w = lane; w < qw1 - qw0; w += SP_WAVE) { LQ[w] = qw[qw0 + w]; if (hasn) NQ[w] = qn ? qn[qw0 + w] : 0u; }
    }
    spw::wave_lds_sync();
    auto base_of = [&](const uint32_t* W, const uint32_t* N, int pos, int w0) {
        const int w = (pos >> 4) - w0; const uint32_t sh = (uint32_t)(pos & 15) << 1;
        if (hasn && ((N[w] >> sh) & 1u)) return 4;
        return (int)((W[w] >> sh) & 3u);
    };
    const int rows = i_hi - i_lo + 1;                       // (the host sized this pair's scratch from the same numbers: af_tb_rows)
    uint8_t* dirs = scratch + off[p];
    AfState H[DPL], E1[DPL], E2[DPL];
#pragma unroll
    for (int c = 0; c < DPL; ++c) H[c] = E1[c] = E2[c] = af_none();
    int bs = 0, bi = -1, bj = -1; uint32_t bm0 = 0, bm1 = 0;
    const int q1 = o.q, e1 = o.e, q2 = o.q2, e2 = o.e2;
    for (int i = i_lo; i <= i_hi; ++i) {
        const int ct = base_of(LT, NT, i, tw0);
        const AfState upH = af_from_upper(H[0]), upE1 = af_from_upper(E1[0]), upE2 = af_from_upper(E2[0]);
        AfState hA[DPL], e1n[DPL], e2n[DPL]; AfKey k1[DPL], k2[DPL]; bool valid[DPL]; uint32_t dir[DPL];
#pragma unroll
        for (int c = 0; c < DPL; ++c) {
            const int idx = lane * DPL + c, j = i + klo + idx;
            valid[c] = (unsigned)j < (unsigned)qlen;
            const AfState hu = c + 1 < DPL ? H[c + 1] : upH, eu = c + 1 < DPL ? E1[c + 1] : upE1, eu2 = c + 1 < DPL ? E2[c + 1] : upE2;
            AfState a1, a2; uint32_t d = AF_D_DIAG;
            { const int eo = hu.s - q1; if (eu.s > eo) { a1 = eu; a1.s = eu.s - e1; d |= AF_D_E1C; } else { a1 = hu; a1.s = eo - e1; } a1.m1 += 1; }
            { const int eo = hu.s - q2; if (eu2.s > eo) { a2 = eu2; a2.s = eu2.s - e2; d |= AF_D_E2C; } else { a2 = hu; a2.s = eo - e2; } a2.m1 += 1; }
            if (a1.s < AF_NEG) a1.s = AF_NEG;
            if (a2.s < AF_NEG) a2.s = AF_NEG;
            AfState h = H[c];
            const int cq = valid[c] ? base_of(LQ, NQ, j, qw0) : 4;
            const bool ambi = ct > 3 || cq > 3;
            const int sub = ambi ? -o.sc_ambi : (ct == cq ? o.a : -o.b);
            if (h.s <= 0) { h.s = 0; h.m1 = 0; h.m0 = ((uint32_t)i << 16) | (uint32_t)(j & 0xFFFF); d |= AF_D_START; }
            h.s += sub; h.m1 += (ambi || ct != cq) ? 1u : 0u;
            if (ambi || ct != cq) d |= AF_D_X;
            if (a1.s > h.s) { h = a1; d = (d & ~7u) | AF_D_E1; }
            if (!valid[c]) { h = af_none(); a1 = af_none(); a2 = af_none(); }
            hA[c] = h; e1n[c] = a1; e2n[c] = a2; dir[c] = d;
            AfState src = h; if (a2.s > src.s) src = a2;
            if (src.s <= 0) { src.s = 0; }
            const bool offer = valid[c] && src.s > 0;
            k1[c].k = offer ? (((uint32_t)(src.s + idx * e1) + AF_BIAS) << 8 | (uint32_t)idx) : 0u; k1[c].m0 = src.m0; k1[c].m1 = src.m1;
            k2[c].k = offer ? (((uint32_t)(src.s + idx * e2) + AF_BIAS) << 8 | (uint32_t)idx) : 0u; k2[c].m0 = src.m0; k2[c].m1 = src.m1;
        }
        AfKey in1 = k1[0], in2 = k2[0];
#pragma unroll
        for (int c = 1; c < DPL; ++c) { in1 = af_max(in1, k1[c]); in2 = af_max(in2, k2[c]); }
        in1 = af_from_lower(af_scan(in1)); in2 = af_from_lower(af_scan(in2));
        uint32_t packed = 0;
#pragma unroll
        for (int c = 0; c < DPL; ++c) {
            const int idx = lane * DPL + c, j = i + klo + idx;
            AfState f1 = af_none(), f2 = af_none(); uint32_t d = dir[c];
            if (in1.k) { const int src_idx = (int)(in1.k & 0xFFu), v = (int)((in1.k >> 8) - AF_BIAS); f1.s = v - q1 - idx * e1; f1.m0 = in1.m0; f1.m1 = in1.m1 + (uint32_t)(idx - src_idx); if (src_idx < idx - 1) d |= AF_D_F1C; }
            if (in2.k) { const int src_idx = (int)(in2.k & 0xFFu), v = (int)((in2.k >> 8) - AF_BIAS); f2.s = v - q2 - idx * e2; f2.m0 = in2.m0; f2.m1 = in2.m1 + (uint32_t)(idx - src_idx); if (src_idx < idx - 1) d |= AF_D_F2C; }
            AfState h = hA[c];
            if (valid[c]) {
                if (f1.s > h.s) { h = f1; d = (d & ~7u) | AF_D_F1; }
                if (e2n[c].s > h.s) { h = e2n[c]; d = (d & ~7u) | AF_D_E2; }
                if (f2.s > h.s) { h = f2; d = (d & ~7u) | AF_D_F2; }
                if (h.s <= 0) { h.s = 0; h.m1 = 0; h.m0 = ((uint32_t)i << 16) | (uint32_t)(j & 0xFFFF); d = (d & ~7u) | AF_D_NONE; }
                const bool better = h.s > bs || (h.s == bs && h.s > 0 && (i + j < bi + bj || (i + j == bi + bj && i < bi)));
                bs = better ? h.s : bs; bi = better ? i : bi; bj = better ? j : bj; bm0 = better ? h.m0 : bm0; bm1 = better ? h.m1 : bm1;
            } else d = AF_D_NONE;
            H[c] = h; E1[c] = e1n[c]; E2[c] = e2n[c];
            in1 = af_max(in1, k1[c]); in2 = af_max(in2, k2[c]);
            packed |= d << (8 * c);
        }
        // the row's records: lane's DPL cells are DPL consecutive bytes -- 64 (one byte a lane) or 256 (one word a lane) contiguous bytes per wave
        if (DPL == 1) dirs[(size_t)(i - i_lo) * BAND + lane] = (uint8_t)packed;
        else ((uint32_t*)dirs)[(size_t)(i - i_lo) * (BAND / 4) + lane] = packed;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const int os = __shfl_xor(bs, d), oi = __shfl_xor(bi, d), oj = __shfl_xor(bj, d);
        const uint32_t om0 = (uint32_t)__shfl_xor((int)bm0, d), om1 = (uint32_t)__shfl_xor((int)bm1, d);
        if (os > bs || (os == bs && os > 0 && (oi + oj < bi + bj || (oi + oj == bi + bj && oi < bi)))) { bs = os; bi = oi; bj = oj; bm0 = om0; bm1 = om1; }
    }
    if (bs <= 0) { if (lane == 0) { out[p] = res; n_cigar[p] = 0; } return; }
    // the walk back.  The rows were written by all lanes and are read by all lanes: they are this workgroup's own, one release / acquire at its scope orders them
    __threadfence_block();
    uint8_t* tile = (uint8_t*)lds;
    uint32_t* ops = (uint32_t*)(dirs + (size_t)rows * BAND);
    const uint32_t ops_cap = 2u * (uint32_t)rows + 2u;
    constexpr int TR = AF_TB_TILE / BAND;
    int ci = bi, cidx = bj - bi - klo, st = 0, done = 0;       // the cell the walk is in (row, diagonal index), its state (0 = H, else AF_D_E1 .. AF_D_F2), 1 = at the start, 2 = lost
    uint32_t n_ops = 0, run_op = 0xF, run_len = 0;
    auto emit = [&](uint32_t op) {
        if (op == run_op) { ++run_len; return; }
        if (run_len) { if (n_ops < ops_cap) ops[n_ops] = run_len << 4 | run_op; ++n_ops; }
        run_op = op; run_len = 1;
    };
    while (!done) {
        const int r1 = ci - i_lo, r0 = r1 - TR + 1 > 0 ? r1 - TR + 1 : 0;
        spw::wave_lds_sync();                               // (the sequences, or the tile before this one, have been read)
        {
            const uint4* src = (const uint4*)(dirs + (size_t)r0 * BAND); const int n16 = (r1 - r0 + 1) * (BAND / 16);
            for (int w = lane; w < n16; w += SP_WAVE) ((uint4*)tile)[w] = src[w];
        }
        spw::wave_lds_sync();
        if (lane == 0) {
            while (true) {
                const int r = ci - i_lo - r0;
                if (r < 0) break;                           // the next tile
                if ((unsigned)cidx >= (unsigned)BAND) { done = 2; break; }
                const uint32_t d = tile[r * BAND + cidx];
                if (st == 0) {
                    const uint32_t h = d & 7u;
                    if (h == AF_D_DIAG || h == AF_D_START) { emit((d & AF_D_X) ? 8u : 7u); --ci; if (h == AF_D_START) { done = 1; break; } continue; }
                    if (h >= AF_D_NONE) { done = 2; break; }
                    st = (int)h;
                }
                if (st == (int)AF_D_E1 || st == (int)AF_D_E2) {            // a base of the target only; the gap came from the cell above: the next diagonal of the row before
                    emit(2u); const bool cont = d & (st == (int)AF_D_E1 ? AF_D_E1C : AF_D_E2C); --ci; ++cidx; if (!cont) st = 0;
                } else {                                                      // a base of the query only; from the cell to the left
                    emit(1u); const bool cont = d & (st == (int)AF_D_F1 ? AF_D_F1C : AF_D_F2C); --cidx; if (!cont) st = 0;
                }
            }
        }
        ci = __shfl(ci, 0); done = __shfl(done, 0);
        if (ci < i_lo && !done) done = 2;
    }
    if (lane == 0) {
        emit(0xE);                                          // closes the last run
        res.score = bs; res.nm = (int32_t)bm1; res.b_start = (int32_t)(bm0 >> 16); res.b_end = bi + 1; res.a_start = (int32_t)(bm0 & 0xFFFFu); res.a_end = bj + 1;
        // a walk that left the band, met a cell nothing ends in or ran out of ops (none of which the forward pass's records allow) is reported, not passed on as a path
        const bool lost = done != 1 || n_ops > ops_cap;
        out[p] = res; n_cigar[p] = lost ? AF_TB_LOST : n_ops;
        const uint32_t n_out = lost ? 0u : (n_ops < stride ? n_ops : stride);
        for (uint32_t k = 0; k < n_out; ++k) cigar[(size_t)p * stride + k] = ops[n_ops - 1 - k];
    }
}

// rows of the target that hold a cell of the pair's band (what both kernels run), 0: nothing to do
inline int64_t af_tb_rows(int tlen, int qlen, int diag, int band) {
    const int64_t klo = -(int64_t)diag - band / 2;
    int64_t i_lo = -(klo + band - 1); if (i_lo < 0) i_lo = 0;
    int64_t i_hi = (int64_t)qlen - 1 - klo; if (i_hi > (int64_t)tlen - 1) i_hi = (int64_t)tlen - 1;
    if (tlen <= 0 || qlen <= 0 || i_lo > i_hi) return 0;
    return i_hi - i_lo + 1;
}

} // namespace

// device-side entry for the library's own callers: pairs and results in device memory
int sp_launch_affine(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const void* d_pairs, uint64_t n_pairs, const sp_affine_opts& o, int band, sp_affine_aln* d_out,
                     const char* prof_name, const uint32_t* d_n_live, const void* d_wins, const void* d_mids) {
    if (n_pairs == 0) return SP_OK;
    if (band != 64 && band != 256) return sp_fail(ctx, SP_ERR_INVALID_ARG, "affine: band must be 64 or 256");
    if (B->max_len > 65535 || A->max_len > 65535) return sp_fail(ctx, SP_ERR_TOO_LONG, "affine: sequences of up to 65,535 bases");
    const int t_words_max = (B->max_len >> 4) + 4;
    const size_t lds_bytes = sizeof(uint32_t) * (size_t)(4 * t_words_max + 2 * (2 * band / 16 + 8));
    ProfScope ps(ctx, prof_name, n_pairs);
    const bool hasn = A->has_n || B->has_n;
#define SP_AF_LAUNCH(D, N) do { \
        (void)hipFuncSetAttribute((const void*)affine_kernel<D, N>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes); \
        hipLaunchKernelGGL((affine_kernel<D, N>), dim3((uint32_t)n_pairs), dim3(64), lds_bytes, ctx->stream, A->view(), B->view(), (const AfPair*)d_pairs, (uint32_t)n_pairs, d_n_live, o, d_out, t_words_max, (const AfWin*)d_wins, (const AfMid*)d_mids); } while (0)
    if (band == 64) { if (hasn) SP_AF_LAUNCH(1, true); else SP_AF_LAUNCH(1, false); }
    else { if (hasn) SP_AF_LAUNCH(4, true); else SP_AF_LAUNCH(4, false); }
#undef SP_AF_LAUNCH
    if (hipGetLastError() != hipSuccess) return sp_fail(ctx, SP_ERR_HIP, "affine launch failed");
    return SP_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Re-score of mappings the library already has, cheaply: most of them need no DP.  A mapping whose edits all stand alone -- at least AF_ISOLATED bases from one
// another and from both ends of the alignment on the window sequence, no ambiguous base in either sequence -- has the same optimum under the two-piece affine scores
// as under unit costs (a lone mismatch or one-base gap is spelled the same way by both, and an edit that far from an end is not clipped: -4 or -8 against at
// least +16): its numbers are the unit-cost numbers, its score a * matches - b * mismatches - (q + e) * gap bases.  (Measured on 1,242 K1 pairs: every mapping
// with all distances >= 12 had identical numbers; 16 is used.)  The others -- one in nine of the K1 winners -- go through the DP above, over the rows around their clustered edits (below).
// The cells are run again with their traceback (sp_cells_kernel<TRACE>) for the positions of the edits; a cell whose second run differs from the alignment the
// caller holds takes the DP as well.
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int AF_ISOLATED = 16;
constexpr int AF_MARGIN = 24;
// what the classification decided for a pair (sp_affine_rescore_mappings_audit): route 0 closed form, 1 the DP over the rows around the clusters, 2 the DP over all rows,
// 3 no mapping; diag = the diagonal (target position - query position) the DP is, or would be, centred on
struct AfAudit { int32_t route, diag; };
// what a stretch of the cell's path costs under the reference's scores: mismatches b each, every RUN of l gap bases min(q + l e, q2 + l e2) (events in path order:
// a run of B-only bases has consecutive positions, a run of A-only bases one position)
__device__ __forceinline__ int af_gap_cost(const sp_affine_opts& o, int l) { const int c1 = o.q + l * o.e, c2 = o.q2 + l * o.e2; return c1 < c2 ? c1 : c2; }
struct AfPathCost {
    int pen = 0, type = -1, pos = 0, run = 0;
    __device__ __forceinline__ void step(const sp_affine_opts& o, int t, int p) {
        if (t == (int)SP_EV_X) { pen += o.b; run = 0; }
        else {
            const bool more = run > 0 && t == type && p == (t == (int)SP_EV_D ? pos + 1 : pos);
            run = more ? run + 1 : 1;
            pen += af_gap_cost(o, run) - (run > 1 ? af_gap_cost(o, run - 1) : 0);
        }
        type = t; pos = p;
    }
};

// d_ref: the alignment the caller holds for each pair (WFA orientation: a_* on Aw, b_* on Bw); cells[x].max_ed < 0: no mapping (score 0).  ENDS: the ends_only rule is compiled in
// (callers that take all six numbers run the kernel without it)
template <bool ENDS>
__global__ void af_classify_kernel(const CellDesc* __restrict__ cells, const sp_aln* __restrict__ ref, const sp_aln* __restrict__ tr, const uint32_t* __restrict__ ev,
                                   uint32_t stride, uint32_t n, int target_is_a, int has_n, sp_affine_opts o, sp_affine_aln* __restrict__ out,
                                   AfPair* __restrict__ todo, uint32_t* __restrict__ todo_at, uint32_t* __restrict__ n_todo, AfWin* __restrict__ wins, AfMid* __restrict__ mids, int band, int windows, int ends_only, AfAudit* __restrict__ audit) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    sp_affine_aln res; res.score = 0; res.nm = 0; res.a_start = res.a_end = res.b_start = res.b_end = 0;
    const CellDesc c = cells[x];
    if (c.max_ed < 0) { out[x] = res; if (audit) { audit[x].route = 3; audit[x].diag = target_is_a ? -c.diag : c.diag; } return; }
    const sp_aln r = ref[x], t = tr[x];
    const int d_mid = ((r.b_start - r.a_start) + (r.b_end - r.a_end)) / 2;         // b_pos - a_pos (WFA orientation)
    const int d_dp = r.ok ? (target_is_a ? -d_mid : d_mid) : (target_is_a ? -c.diag : c.diag);      // in the affine kernel's order; a lost cell: the cell's own diagonal
    bool simple = !has_n && r.ok && t.ok && t.nm == r.nm && t.a_start == r.a_start && t.a_end == r.a_end && t.b_start == r.b_start && t.b_end == r.b_end && (uint32_t)r.nm <= stride;
    const bool traced = simple;
    int nx = 0, ngap = 0, gap_cost = -1;                                     // (gap_cost >= 0: the gap bases' cost in true runs, ends_only)
    if (simple) {
        const uint32_t* e = ev + (size_t)x * stride;
        int prev = -(1 << 29);
        for (int k = 0; k < r.nm && simple; ++k) {
            const uint32_t w = e[k]; const int pos = (int)(w & 0x3FFFFFFFu), type = (int)(w >> 30);
            const int gap = pos > prev ? pos - prev : prev - pos;
            if (k > 0 && gap < AF_ISOLATED) simple = false;
            if (pos - r.b_start < AF_ISOLATED || r.b_end - pos < AF_ISOLATED) simple = false;
            if (type == (int)SP_EV_X) ++nx; else ++ngap;
            prev = pos;
        }
    }
    // ends_only: the caller takes the mapping's EXTENT (where minimap2's end clipping leaves its two ends) and nothing else.  An end is clipped where the alignment from it
    // inwards does not pay, so that is what is tested: the cell's path is scored the reference's way (mismatches, gap RUNS at min(q + l e, q2 + l e2)) from the head to
    // behind every edit and from the tail to in front of every edit.  That is a lower bound of what the DP finds between the same two points ON THAT PATH; where it stays at or above
    // `clear` -- the least the lone-edit rule above lets stand, AF_ISOLATED matches less a one-base gap -- the end is taken not to be clipped.  This is a criterion held by
    // tests (tests/test_gpu_rescore_shortcuts.py against oracle/affine.c), not a proof: it does not exclude an optimum on another path with another extent, as repeats could
    // offer one.  A mapping with both ends so cleared keeps the cell's extent without a DP, whatever its edits in between (count and score are then the unit-cost spelling's under true gap-run costs: positive, and
    // such a caller uses neither).  An end that is not cleared takes the DP from that end to behind the last edit that is in doubt (kh: the last one whose score from the head
    // falls below it, kt: the first one whose score to the tail does), and so does an end with an edit that does not stand alone within ends_only bases of it; both
    // stretches run on to the first AF_MARGIN + AF_ISOLATED bases without an edit, what lies between them enters in closed form, and two that meet are the DP over all rows --
    // as is a path that leaves the diagonals of the DP's band, whose optimum is then another alignment.
    // An HLA read is 40 - 100 clustered edits from the reference: the DP over all of its rows was 17.5 ms per 10,000 reads.
    int kh = -1, kt = r.nm;
    if (ENDS && ends_only > 0 && traced && !simple && r.nm > 0) {
        const uint32_t* e = ev + (size_t)x * stride;
        const int clear = o.a * AF_ISOLATED - af_gap_cost(o, 1);
        AfPathCost pc; int nxd = 0, total = 0, drift = 0;
        bool in_band = true;                                                   // the path stays on the diagonals the DP would run: otherwise the DP's optimum is not this path's
        nx = 0; ngap = 0;
        for (int pass = 0; pass < 2; ++pass) {
            // pass 0: the path's score from the head to behind edit k, and the whole path's (total); pass 1: from in front of edit k to the tail = total - (the score up to there)
            pc = AfPathCost(); nxd = 0;
            for (int k = 0; k < r.nm; ++k) {
                const uint32_t w = e[k]; const int pos = (int)(w & 0x3FFFFFFFu), type = (int)(w >> 30);
                const int before = o.a * (pos - r.b_start - nxd) - pc.pen;
                pc.step(o, type, pos);
                if (type != (int)SP_EV_I) ++nxd;
                if (pass == 0) {
                    if (type == (int)SP_EV_X) ++nx; else ++ngap;
                    drift += type == (int)SP_EV_D ? 1 : type == (int)SP_EV_I ? -1 : 0;
                    const int off = (r.b_start - r.a_start) + drift - d_mid;
                    if (off <= -(band / 2 - 2) || off >= band / 2 - 2) in_band = false;
                    const int prev = k > 0 ? (int)(e[k - 1] & 0x3FFFFFFFu) : -(1 << 29), next = k + 1 < r.nm ? (int)(e[k + 1] & 0x3FFFFFFFu) : (1 << 29);
                    const bool lone = pos - prev >= AF_ISOLATED && next - pos >= AF_ISOLATED && pos - r.b_start >= AF_ISOLATED && r.b_end - pos >= AF_ISOLATED;
                    if (o.a * (pos - r.b_start - (nxd - (type != (int)SP_EV_I ? 1 : 0))) - pc.pen < clear || (!lone && pos - r.b_start < ends_only)) kh = k;
                    if (!lone && r.b_end - pos < ends_only && k < kt) kt = k;
                } else if (total - before < clear && k < kt) kt = k;
            }
            if (pass == 0) total = o.a * (r.b_end - r.b_start - nxd) - pc.pen;
        }
        if (!in_band) { kh = r.nm - 1; kt = 0; }                              // (the two stretches meet: the DP over all rows)
        if (kh < 0 && kt == r.nm) { simple = true; gap_cost = pc.pen - o.b * nx; }
    }
    if (simple) {
        // columns: M matches, X mismatches, gap bases on either side; a_span = M + X + (A-only bases), b_span = M + X + (B-only bases), gap bases = ngap
        const int a_span = r.a_end - r.a_start, b_span = r.b_end - r.b_start;
        const int m2 = a_span + b_span - 2 * nx - ngap;                          // = 2 M
        const int M = m2 / 2;
        res.score = o.a * M - o.b * nx - (gap_cost >= 0 ? gap_cost : (o.q + o.e) * ngap); res.nm = r.nm;
        if (target_is_a) { res.b_start = r.a_start; res.b_end = r.a_end; res.a_start = r.b_start; res.a_end = r.b_end; }
        else { res.a_start = r.a_start; res.a_end = r.a_end; res.b_start = r.b_start; res.b_end = r.b_end; }
        out[x] = res;
        if (audit) { audit[x].route = 0; audit[x].diag = d_dp; }
        return;
    }
    // the DP: query / target in the affine kernel's order, on the diagonal the alignment lies on
    const uint32_t at = atomicAdd(n_todo, 1u);
    AfPair p;
    if (target_is_a) { p.a = c.b; p.b = c.a; } else { p.a = c.a; p.b = c.b; }
    p.diag = d_dp; p.pad = 0;
    todo[at] = p; todo_at[at] = x;
    // the rows the DP has to run: for every run of edits that do not stand alone, from AF_MARGIN bases before its first edit to AF_MARGIN behind its last one, both ends
    // moved outwards until no other edit lies within AF_ISOLATED bases of them; what lies before, between and behind these stretches is spelled by both scoring schemes
    // the same way (the argument above) and enters in closed form.  An end that would come within AF_ISOLATED bases of the alignment's own end is left to the DP, two
    // stretches less than AF_ISOLATED apart are one, and so are the stretches beyond the AF_MAXMID + 1 a pair can have.
    AfWin w; w.r0 = -1; w.r1 = -1; w.idx_in = w.idx_out = 0; w.s_in = w.nm_in = w.d_score = w.d_nm = w.end_t = w.end_q = w.n_mid = 0; w.start_cell = 0;
    if (traced && windows && r.nm > 0) {
        const uint32_t* e = ev + (size_t)x * stride;
        auto pos_of = [&](int k) { return (int)(e[k] & 0x3FFFFFFFu); };
        int wF[AF_MAXMID + 1], wL[AF_MAXMID + 1], wIn[AF_MAXMID + 1], wOut[AF_MAXMID + 1], nw = 0;
        const bool ends_head = ENDS && kh >= 0, ends_tail = ENDS && kt < r.nm;
        if (ends_head || ends_tail) {
            // (ends_only: at most two stretches, one per end that was not shown to stand)
            if (ends_head) { while (kh + 1 < r.nm && pos_of(kh + 1) - pos_of(kh) < AF_MARGIN + AF_ISOLATED) ++kh; }
            if (ends_tail) { while (kt > 0 && pos_of(kt) - pos_of(kt - 1) < AF_MARGIN + AF_ISOLATED) --kt; }
            if (kh < kt) {
                if (ends_head) { wF[nw] = 0; wL[nw] = kh; wIn[nw] = pos_of(0) - AF_MARGIN; wOut[nw] = pos_of(kh) + AF_MARGIN; ++nw; }
                if (ends_tail) { wF[nw] = kt; wL[nw] = r.nm - 1; wIn[nw] = pos_of(kt) - AF_MARGIN; wOut[nw] = pos_of(r.nm - 1) + AF_MARGIN; ++nw; }
            }                                                                                      // (else the two meet: the DP over all rows)
        } else
        for (int k = 0; k < r.nm; ++k) {
            const int pos = pos_of(k);
            const bool lone = !(pos - r.b_start < AF_ISOLATED || r.b_end - pos < AF_ISOLATED) && !(k > 0 && pos - pos_of(k - 1) < AF_ISOLATED) && !(k + 1 < r.nm && pos_of(k + 1) - pos < AF_ISOLATED);
            if (lone) continue;
            int kF = k, kL = k;
            const int floor_k = nw ? wL[nw - 1] + 1 : 0;
            int entry = pos_of(kF) - AF_MARGIN;
            while (kF > floor_k && pos_of(kF - 1) > entry - AF_ISOLATED) { --kF; entry = pos_of(kF) - AF_MARGIN; }
            int leave = pos_of(kL) + AF_MARGIN;
            while (kL + 1 < r.nm && pos_of(kL + 1) < leave + AF_ISOLATED) { ++kL; leave = pos_of(kL) + AF_MARGIN; }
            if (nw && (entry - wOut[nw - 1] < AF_ISOLATED || nw == AF_MAXMID + 1)) { wL[nw - 1] = kL; wOut[nw - 1] = leave; }
            else { wF[nw] = kF; wL[nw] = kL; wIn[nw] = entry; wOut[nw] = leave; ++nw; }
            k = kL;
        }
        if (nw > 0) {
            const int klo = -p.diag - band / 2;
            // the walk along the alignment: (i, j) = the next bases of the streamed and the window sequence; cx / cd / ci = the lone edits since the last stretch
            // (pc.pen: what they cost the reference's way, gap runs as runs -- between the two stretches of an ends_only pair the edits need not stand alone)
            int i = r.a_start, j = r.b_start, cx = 0, cd = 0, ci = 0, k = 0; AfPathCost pc;
            auto piece_cost = [&]() { return ENDS ? pc.pen : o.b * cx + (o.q + o.e) * (cd + ci); };
            auto step_to = [&](int k2) { const int pos = pos_of(k2), type = (int)(e[k2] >> 30); if (ENDS) pc.step(o, type, pos); i += pos - j; j = pos; if (type == (int)SP_EV_X) { ++i; ++j; ++cx; } else if (type == (int)SP_EV_D) { ++j; ++cd; } else { ++i; ++ci; } };
            AfMid* mid = mids + (size_t)at * AF_MAXMID;
            int out_t = 0, out_idx = 0, out_b = 0; bool have_out = false;
            for (int v = 0; v < nw; ++v) {
                for (; k < wF[v]; ++k) step_to(k);
                {
                    const int ia = i + (wIn[v] - j), jb = wIn[v];                                   // the first cell the DP scores; the one before it is a match on the same diagonal
                    const int t_in = target_is_a ? ia : jb, q_in = target_is_a ? jb : ia;
                    const int idx = (q_in - t_in) - klo;
                    const bool fits = idx >= 0 && idx < band && t_in >= 1 && q_in >= 1;
                    if (v == 0) {
                        if (wIn[0] - r.b_start >= AF_ISOLATED && fits) {
                            w.r0 = t_in; w.idx_in = idx;
                            w.s_in = o.a * ((wIn[0] - r.b_start) - cx - cd) - piece_cost(); w.nm_in = cx + cd + ci;
                            const int ts = target_is_a ? r.a_start : r.b_start, qs = target_is_a ? r.b_start : r.a_start;
                            w.start_cell = ((uint32_t)ts << 16) | (uint32_t)(qs & 0xFFFF);
                        }
                    } else if (have_out && fits && t_in > out_t + 1) {
                        AfMid m; m.r_exit = out_t; m.idx_out = out_idx; m.r_entry = t_in; m.idx_in = idx;
                        m.d_score = o.a * ((wIn[v] - out_b - 1) - cx - cd) - piece_cost(); m.d_nm = cx + cd + ci;
                        mid[w.n_mid++] = m;
                    }
                }
                for (; k <= wL[v]; ++k) step_to(k);
                cx = cd = ci = 0; pc.pen = 0;
                {
                    const int ia = i + (wOut[v] - j), jb = wOut[v];                                 // a matching cell AF_MARGIN behind the last edit of the stretch
                    const int t_out = target_is_a ? ia : jb, q_out = target_is_a ? jb : ia;
                    const int idx = (q_out - t_out) - klo;
                    have_out = idx >= 0 && idx < band && wOut[v] >= j;
                    out_t = t_out; out_idx = idx; out_b = wOut[v];
                }
            }
            if (have_out && r.b_end - out_b >= AF_ISOLATED) {
                for (; k < r.nm; ++k) step_to(k);
                w.r1 = out_t; w.idx_out = out_idx;
                w.d_score = o.a * ((r.b_end - out_b - 1) - cx - cd) - piece_cost(); w.d_nm = cx + cd + ci;
                w.end_t = target_is_a ? r.a_end : r.b_end; w.end_q = target_is_a ? r.b_end : r.a_end;
            }
        }
    }
    wins[at] = w;
    if (audit) { audit[x].route = (w.r0 >= 0 || w.r1 >= 0 || w.n_mid > 0) ? 1 : 2; audit[x].diag = d_dp; }
}
__global__ void af_scatter_kernel(const sp_affine_aln* __restrict__ part, const uint32_t* __restrict__ todo_at, const uint32_t* __restrict__ n_todo, sp_affine_aln* __restrict__ out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < *n_todo) out[todo_at[k]] = part[k];
}

// the mappings of cells (WFA orientation: Aw streamed, Bw window; d_ref = the alignments the caller holds) re-scored into d_out (a_* on minimap2's query, b_* on its target:
// target_is_a tells which of the two sets is the target); everything stays on the device
int sp_rescore_mappings(sp_ctx* ctx, const sp_seqset* Aw, const sp_seqset* Bw, const CellDesc* d_cells, const sp_aln* d_ref, uint64_t n, bool target_is_a,
                        const sp_affine_opts& o, int band, sp_affine_aln* d_out, const char* prefix, uint32_t stride, int trace_retry_wide, const sp_aln* d_tr_in, const uint32_t* d_ev_in, int ends_only, int windows, void* d_audit) {
    if (n == 0) return SP_OK;
    const std::string pre(prefix);
    static std::mutex names_lock; static std::set<std::string> names;                 // (the profiler keeps the pointers it is given)
    auto stable = [&](const std::string& n2) { std::lock_guard<std::mutex> g(names_lock); return names.insert(n2).first->c_str(); };
    // (d_tr_in / d_ev_in: the caller ran its cells with their traceback itself -- d_ref's own alignments and their edit events, `stride` words each: no second run of the cells)
    const sp_aln* d_tr = d_tr_in ? d_tr_in : (const sp_aln*)sp_pool(ctx, (pre + "_tr").c_str(), n * sizeof(sp_aln));
    const uint32_t* d_ev = d_ev_in ? d_ev_in : (const uint32_t*)sp_pool(ctx, (pre + "_ev").c_str(), n * (size_t)stride * 4);
    AfPair* d_todo = (AfPair*)sp_pool(ctx, (pre + "_todo").c_str(), n * sizeof(AfPair));
    uint32_t* d_at = (uint32_t*)sp_pool(ctx, (pre + "_at").c_str(), n * 4 + 64);
    sp_affine_aln* d_part = (sp_affine_aln*)sp_pool(ctx, (pre + "_part").c_str(), n * sizeof(sp_affine_aln));
    AfWin* d_win = (AfWin*)sp_pool(ctx, (pre + "_win").c_str(), n * sizeof(AfWin));
    AfMid* d_mid = (AfMid*)sp_pool(ctx, (pre + "_mid").c_str(), n * sizeof(AfMid) * AF_MAXMID);
    if (!d_tr || !d_ev || !d_todo || !d_at || !d_part || !d_win || !d_mid) return sp_fail(ctx, SP_ERR_OUT_OF_MEMORY, "rescore buffers");
    uint32_t* d_n = d_at + n;
    (void)hipMemsetAsync(d_n, 0, 4, ctx->stream);
    int rc = SP_OK;
    if (!d_tr_in) rc = sp_launch_cells(ctx, Aw, Bw, d_cells, n, const_cast<sp_aln*>(d_tr), const_cast<uint32_t*>(d_ev), stride, stable(pre + "_trace"), trace_retry_wide);
    if (rc != SP_OK) return rc;
    auto* classify = ends_only > 0 ? af_classify_kernel<true> : af_classify_kernel<false>;
    hipLaunchKernelGGL(classify, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_cells, d_ref, d_tr, d_ev, stride, (uint32_t)n, target_is_a ? 1 : 0,
                       (Aw->has_n || Bw->has_n) ? 1 : 0, o, d_out, d_todo, d_at, d_n, d_win, d_mid, band, windows < 0 ? (ctx->mm2_rescore == 2 ? 0 : 1) : windows, ends_only, (AfAudit*)d_audit);
    // the DP over the list the classification left: launched for every pair, the workgroups behind the list's end return at once (no host round trip for the count)
    rc = sp_launch_affine(ctx, target_is_a ? Bw : Aw, target_is_a ? Aw : Bw, d_todo, n, o, band, d_part, stable(pre + "_dp"), d_n, d_win, d_mid);
    if (rc != SP_OK) return rc;
    hipLaunchKernelGGL(af_scatter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_part, d_at, d_n, d_out);
    if (ctx->profile_rescore_counts && ctx->profiling) {
        // (a measuring run: how many pairs the classification left to the DP -- one word fetched, the host waits for the stream)
        uint32_t n_dp = 0;
        SP_HIP_CHECK(ctx, hipMemcpyAsync(&n_dp, d_n, 4, hipMemcpyDeviceToHost, ctx->stream));
        SP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        auto& e = ctx->prof[pre + "_dp_pairs"]; e.cells += n_dp; e.launches += 1;
    }
    return SP_OK;
}

extern "C" int32_t sp_affine_rescore_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_opts* opts,
                                           int32_t band, sp_affine_aln* out) {
    if (!ctx || !A || !B || !opts || (n_pairs && (!pairs || !out))) return SP_ERR_INVALID_ARG;
    if (n_pairs == 0) return SP_OK;
    if (n_pairs > 0xFFFFFFFFull) return sp_fail(ctx, SP_ERR_INVALID_ARG, "affine: too many pairs");
    (void)hipSetDevice(ctx->device);
    for (uint64_t i = 0; i < n_pairs; ++i) if (pairs[i].a >= A->n || pairs[i].b >= B->n) return sp_fail(ctx, SP_ERR_INVALID_ARG, "affine: index out of range");
    static_assert(sizeof(sp_pair) == sizeof(AfPair), "pair layout");
    void* d_pairs = sp_pool(ctx, "affine_pairs", n_pairs * sizeof(sp_pair));
    sp_affine_aln* d_out = (sp_affine_aln*)sp_pool(ctx, "affine_out", n_pairs * sizeof(sp_affine_aln));
    if (!d_pairs || !d_out) return sp_fail(ctx, SP_ERR_OUT_OF_MEMORY, "affine buffers");
    SP_HIP_CHECK(ctx, hipMemcpyAsync(d_pairs, pairs, n_pairs * sizeof(sp_pair), hipMemcpyHostToDevice, ctx->stream));
    const int rc = sp_launch_affine(ctx, A, B, d_pairs, n_pairs, *opts, band, d_out, "affine_rescore", nullptr, nullptr, nullptr);
    if (rc != SP_OK) return rc;
    SP_HIP_CHECK(ctx, hipMemcpyAsync(out, d_out, n_pairs * sizeof(sp_affine_aln), hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
}

// sp_rescore_mappings as the library's own callers run it, for pairs a test hands in: each pair's cell (what sp_align_batch runs for it) is the alignment "the caller
// holds", the re-score takes exactly the knobs given, and what the classification decided comes back beside the numbers
extern "C" int32_t sp_affine_rescore_mappings_audit(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_opts* opts,
                                                    int32_t band, int32_t target_is_a, uint32_t events_stride, int32_t windows, int32_t ends_only, sp_affine_aln* out,
                                                    int32_t* route, int32_t* diag) {
    if (!ctx || !A || !B || !opts || (n_pairs && (!pairs || !out || !route || !diag))) return SP_ERR_INVALID_ARG;
    if (n_pairs == 0) return SP_OK;
    if (n_pairs > 0xFFFFFFFFull) return sp_fail(ctx, SP_ERR_INVALID_ARG, "rescore audit: too many pairs");
    if (events_stride == 0 || events_stride > SP_MAX_ED + 1) return sp_fail(ctx, SP_ERR_INVALID_ARG, "rescore audit: events_stride must be 1..SP_MAX_ED + 1");
    if (ends_only < 0) return sp_fail(ctx, SP_ERR_INVALID_ARG, "rescore audit: ends_only must be >= 0");
    (void)hipSetDevice(ctx->device);
    std::vector<CellDesc> cells(n_pairs);
    for (uint64_t i = 0; i < n_pairs; ++i) {
        if (pairs[i].a >= A->n || pairs[i].b >= B->n) return sp_fail(ctx, SP_ERR_INVALID_ARG, "rescore audit: index out of range");
        if (pairs[i].max_ed > SP_MAX_ED) return sp_fail(ctx, SP_ERR_INVALID_ARG, "rescore audit: max_ed must be <= SP_MAX_ED (< 0: no mapping)");
        cells[i] = CellDesc{pairs[i].a, pairs[i].b, pairs[i].diag, pairs[i].max_ed, 0, -1};
    }
    CellDesc* d_cells = (CellDesc*)sp_pool(ctx, "af_audit_cells", n_pairs * sizeof(CellDesc));
    sp_aln* d_ref = (sp_aln*)sp_pool(ctx, "af_audit_ref", n_pairs * sizeof(sp_aln));
    sp_affine_aln* d_out = (sp_affine_aln*)sp_pool(ctx, "af_audit_out", n_pairs * sizeof(sp_affine_aln));
    AfAudit* d_audit = (AfAudit*)sp_pool(ctx, "af_audit_route", n_pairs * sizeof(AfAudit));
    if (!d_cells || !d_ref || !d_out || !d_audit) return sp_fail(ctx, SP_ERR_OUT_OF_MEMORY, "rescore audit buffers");
    SP_HIP_CHECK(ctx, hipMemcpyAsync(d_cells, cells.data(), n_pairs * sizeof(CellDesc), hipMemcpyHostToDevice, ctx->stream));
    SP_HIP_CHECK(ctx, hipMemsetAsync(d_ref, 0, n_pairs * sizeof(sp_aln), ctx->stream));       // (a cell with max_ed < 0 is not run: ok = 0)
    int rc = sp_launch_cells(ctx, A, B, d_cells, n_pairs, d_ref, nullptr, 0, "af_audit_cells", 2);
    if (rc != SP_OK) return rc;
    rc = sp_rescore_mappings(ctx, A, B, d_cells, d_ref, n_pairs, target_is_a != 0, *opts, band, d_out, "af_audit", events_stride, 2, nullptr, nullptr, ends_only, windows ? 1 : 0, d_audit);
    if (rc != SP_OK) return rc;
    std::vector<AfAudit> au(n_pairs);
    SP_HIP_CHECK(ctx, hipMemcpyAsync(out, d_out, n_pairs * sizeof(sp_affine_aln), hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP_CHECK(ctx, hipMemcpyAsync(au.data(), d_audit, n_pairs * sizeof(AfAudit), hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (uint64_t i = 0; i < n_pairs; ++i) { route[i] = au[i].route; diag[i] = au[i].diag; }
    return SP_OK;
}

// The direction rows of a batch would be a few GB at once (10,000 reads against 3.5 - 16 kb alleles: rows x 64 bytes each), so the batch runs in chunks of pairs
// whose rows fit AF_TB_BUDGET bytes of one pooled scratch (a single pair is at most 65,535 rows x 256 bytes = 16 MB); the launches of a call follow one another on
// the context's stream and reuse it.
constexpr size_t AF_TB_BUDGET = 512ull << 20;

extern "C" int32_t sp_affine_align_batch(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const sp_pair* pairs, uint64_t n_pairs, const sp_affine_opts* opts,
                                         int32_t band, sp_affine_aln* out, uint32_t* cigar, uint32_t cigar_stride, uint32_t* n_cigar) {
    if (!ctx || !A || !B || !opts || (n_pairs && (!pairs || !out || !n_cigar || (cigar_stride && !cigar)))) return SP_ERR_INVALID_ARG;
    if (n_pairs == 0) return SP_OK;
    if (n_pairs > 0xFFFFFFFFull) return sp_fail(ctx, SP_ERR_INVALID_ARG, "affine: too many pairs");
    if (band != 64 && band != 256) return sp_fail(ctx, SP_ERR_INVALID_ARG, "affine: band must be 64 or 256");
    if (B->max_len > 65535 || A->max_len > 65535) return sp_fail(ctx, SP_ERR_TOO_LONG, "affine: sequences of up to 65,535 bases");
    (void)hipSetDevice(ctx->device);
    for (uint64_t i = 0; i < n_pairs; ++i) if (pairs[i].a >= A->n || pairs[i].b >= B->n) return sp_fail(ctx, SP_ERR_INVALID_ARG, "affine: index out of range");
    // every pair's place in the scratch of its chunk: rows x band direction bytes, then 2 rows + 2 op words
    std::vector<uint64_t> off(n_pairs); std::vector<uint64_t> chunk_end;         // chunk_end: one past the last pair of each chunk
    size_t used = 0, largest = 0;
    for (uint64_t i = 0; i < n_pairs; ++i) {
        const int64_t rows = pairs[i].max_ed < 0 ? 0 : af_tb_rows(B->h_len[pairs[i].b], A->h_len[pairs[i].a], pairs[i].diag, band);
        const size_t bytes = rows ? (((size_t)rows * band + ((size_t)2 * rows + 2) * 4 + 15) & ~(size_t)15) : 0;
        if (used && used + bytes > AF_TB_BUDGET) { chunk_end.push_back(i); used = 0; }
        off[i] = used; used += bytes; largest = std::max(largest, used);
    }
    chunk_end.push_back(n_pairs);
    void* d_pairs = sp_pool(ctx, "affine_pairs", n_pairs * sizeof(sp_pair));
    sp_affine_aln* d_out = (sp_affine_aln*)sp_pool(ctx, "affine_out", n_pairs * sizeof(sp_affine_aln));
    uint64_t* d_off = (uint64_t*)sp_pool(ctx, "affine_tb_off", n_pairs * 8);
    uint32_t* d_nc = (uint32_t*)sp_pool(ctx, "affine_tb_n", n_pairs * 4);
    uint32_t* d_cg = (uint32_t*)sp_pool(ctx, "affine_tb_cigar", std::max<size_t>(16, n_pairs * (size_t)cigar_stride * 4));
    if (!d_pairs || !d_out || !d_off || !d_nc || !d_cg) return sp_fail(ctx, SP_ERR_OUT_OF_MEMORY, "affine traceback buffers");
    // the direction rows are the call's own, not the pool's: up to AF_TB_BUDGET bytes that a context which has written one debug file should not keep
    struct Rows { uint8_t* p = nullptr; ~Rows() { if (p) (void)hipFree(p); } } rows_buf;
    if (hipMalloc((void**)&rows_buf.p, std::max<size_t>(16, largest)) != hipSuccess) { rows_buf.p = nullptr; return sp_fail(ctx, SP_ERR_OUT_OF_MEMORY, "affine traceback: direction rows"); }
    uint8_t* d_scr = rows_buf.p;
    SP_HIP_CHECK(ctx, hipMemcpyAsync(d_pairs, pairs, n_pairs * sizeof(sp_pair), hipMemcpyHostToDevice, ctx->stream));
    SP_HIP_CHECK(ctx, hipMemcpyAsync(d_off, off.data(), n_pairs * 8, hipMemcpyHostToDevice, ctx->stream));
    const int t_words_max = (B->max_len >> 4) + 4;
    const size_t lds_bytes = std::max<size_t>(AF_TB_TILE, sizeof(uint32_t) * (size_t)(4 * t_words_max + 2 * (2 * band / 16 + 8)));
    const bool hasn = A->has_n || B->has_n;
#define SP_AF_TB_ATTR(D, N) (void)hipFuncSetAttribute((const void*)affine_tb_kernel<D, N>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes)
    if (band == 64) { if (hasn) SP_AF_TB_ATTR(1, true); else SP_AF_TB_ATTR(1, false); }
    else { if (hasn) SP_AF_TB_ATTR(4, true); else SP_AF_TB_ATTR(4, false); }
    uint64_t p0 = 0;
    for (const uint64_t p1 : chunk_end) {
        const uint32_t n = (uint32_t)(p1 - p0);
        ProfScope ps(ctx, "affine_align", n);
#define SP_AF_TB_LAUNCH(D, N) do { \
        hipLaunchKernelGGL((affine_tb_kernel<D, N>), dim3(n), dim3(64), lds_bytes, ctx->stream, A->view(), B->view(), (const AfPair*)d_pairs + p0, n, *opts, d_out + p0, t_words_max, \
                           d_scr, d_off + p0, d_cg + p0 * cigar_stride, cigar_stride, d_nc + p0); } while (0)
        if (band == 64) { if (hasn) SP_AF_TB_LAUNCH(1, true); else SP_AF_TB_LAUNCH(1, false); }
        else { if (hasn) SP_AF_TB_LAUNCH(4, true); else SP_AF_TB_LAUNCH(4, false); }
#undef SP_AF_TB_LAUNCH
#undef SP_AF_TB_ATTR
        if (hipGetLastError() != hipSuccess) return sp_fail(ctx, SP_ERR_HIP, "affine traceback launch failed");
        p0 = p1;
    }
    SP_HIP_CHECK(ctx, hipMemcpyAsync(out, d_out, n_pairs * sizeof(sp_affine_aln), hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP_CHECK(ctx, hipMemcpyAsync(n_cigar, d_nc, n_pairs * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (cigar_stride) SP_HIP_CHECK(ctx, hipMemcpyAsync(cigar, d_cg, n_pairs * (size_t)cigar_stride * 4, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (uint64_t i = 0; i < n_pairs; ++i)
        if (n_cigar[i] == AF_TB_LOST) { n_cigar[i] = 0; return sp_fail(ctx, SP_ERR_HIP, "affine traceback: the walk of pair " + std::to_string(i) + " did not reach the cell its path started in"); }
    return SP_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// The K2 map (sp_hla_map_consensus): the same alignment as sp_affine_align_batch on 64 diagonals, for the thousands of (allele, consensus) pairs of a K2 call, WITHOUT
// a direction byte per cell in global memory.  A persistent grid of single-wave workgroups strides over the pair list; what a wave keeps outside its registers and
// LDS belongs to its SLOT in the grid, not to a pair, so the scratch of a call is (slots x a bound per slot) whatever the number of pairs or cells:
//   forward  the rows of affine_tb_kernel's forward pass (DPL = 1) on scores alone -- every decision of that pass compares scores, the counters and start cells only ride
//            along -- for the best cell; before every AF_MAP_ROWS-th row the wave leaves its H / E1 / E2 scores in its slot's checkpoint list: 768 bytes a checkpoint
//   walk     from the best cell block by block backwards: the wave runs the block's rows again from its checkpoint -- scores only, the same comparisons, so the same
//            decisions -- writing the direction bytes of affine_tb_kernel's format into an LDS tile of AF_MAP_ROWS x 64 bytes (8 KB, beside the packed sequences), and
//            lane 0 follows them as affine_tb_kernel's walk does.  Rows behind the cell the walk is in are not run again.
//   ops      written backwards into the slot's ring of AF_MAP_RING words, then copied in forward order to a place the wave takes from a bump cursor in ONE compact op
//            buffer for the whole launch (op_off[p]; AF_MAP_NO_OPS: the buffer or the ring was too small -- n_cigar[p] is the true count either way and the cursor the
//            space the launch asked for in all, so the host grows the pooled buffer and launches again).
// Why the result is affine_tb_kernel's: every decision of the DP -- which predecessor a state takes, whether a gap continues, which cell is best -- compares scores, and both
// runs here make those comparisons on the same scores in the same order; the counters and start cells affine_tb_kernel carries along take no part in them.  So the best
// cell, the direction bytes and hence the walk and its ops are the same; NM is the number of the path's columns that are not '=' and the start cell is the cell the walk
// ends in, which is what the carried counters add up to along that same path.
//
// The wide instance (DPL = 4: 256 diagonals, sp_align_pileup_band_batch and the second try of sp_hla_consensus_support) is the same kernel with affine_tb_kernel<4>'s
// cell layout: lane l holds diagonals 4 l .. 4 l + 3, the upper neighbour of its last diagonal is lane l + 1's first, the F scan runs over the maximum of the lane's
// four keys and is finished inside the lane in diagonal order (the diagonal index, 0 .. 255, still fills the key's low 8 bits).  The argument above carries over word
// for word with affine_tb_kernel<4> in the place of affine_tb_kernel<1>: H / E1 / E2 are int[4], scores only, and every comparison is the one that kernel makes, in its
// order.  A row of direction bytes is 256 bytes, a lane's four cells one 32-bit LDS store (as affine_tb_kernel<4> stores them to global memory), lane 0's walk is the
// same with that row pitch, and a checkpoint is 3 x 256 words = 3 KB.
//   rows per block   AF_MAP_ROWS_WIDE = SP_ALIGN_PILEUP_WIDE_ROWS = 128: a 32 KB tile
//   slots per CU     AF_MAP_SLOTS_WIDE = 4 (the 64-diagonal instance: 8): one wave per SIMD
//   LDS              32,768 + target length + 384 bytes: 36.6 KB for a 3.5 kb target (four workgroups a CU), 49.2 KB for 16 kb (three)
//   pooled scratch   slots x ((max target / 128 + 2) checkpoints x 3 KB + 16 KB ring); 1,024 slots on 256 CUs: 107 MB for 3.5 kb targets, 416 MB for 16 kb ones,
//                    whatever the number of pairs (the 64-diagonal instance: 2,048 slots x 768-byte checkpoints = 79 MB and 233 MB)
// 64 rows per block halve the tile, but the checkpoints double and only buy occupancy if the slots double as well: four times the checkpoint scratch.  That
// alternative has not been measured; the choice rests on these figures (profiles/support/wide_map.txt: 16.6 ms against affine_tb_kernel<4>'s 37.6).
// ------------------------------------------------------------------------------------------------------------------------------
namespace {

constexpr int AF_MAP_ROWS = 128;
constexpr int AF_MAP_ROWS_WIDE = SP_ALIGN_PILEUP_WIDE_ROWS;
constexpr int AF_MAP_SLOTS = 8, AF_MAP_SLOTS_WIDE = 4;     // workgroups of the persistent grid per CU
constexpr uint32_t AF_MAP_RING = 4096;
constexpr uint64_t AF_MAP_NO_OPS = ~0ull;
static_assert((AF_MAP_ROWS & (AF_MAP_ROWS - 1)) == 0 && (AF_MAP_ROWS_WIDE & (AF_MAP_ROWS_WIDE - 1)) == 0, "rows per block: a power of two");

// af_scan on the key alone
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t af_map_dpp(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false); }
__device__ __forceinline__ uint32_t af_map_max(uint32_t a, uint32_t b) { return b > a ? b : a; }
__device__ __forceinline__ uint32_t af_map_scan(uint32_t v) {
    v = af_map_max(v, af_map_dpp<0x111, 0xf>(v));
    v = af_map_max(v, af_map_dpp<0x112, 0xf>(v));
    v = af_map_max(v, af_map_dpp<0x114, 0xf>(v));
    v = af_map_max(v, af_map_dpp<0x118, 0xf>(v));
    v = af_map_max(v, af_map_dpp<0x142, 0xa>(v));
    v = af_map_max(v, af_map_dpp<0x143, 0xc>(v));
    return v;
}

// n_live: the launch runs min(*n_live, n_pairs) entries (a count a kernel before it left); list: entry k is pair list[k], its results go to that pair's own index
template <int DPL, bool HASN>
__global__ __launch_bounds__(64) void affine_map_kernel(SeqSetView A, SeqSetView B, const AfPair* __restrict__ pairs, uint32_t n_pairs, const uint32_t* __restrict__ n_live,
                                                         const uint32_t* __restrict__ list, sp_affine_opts o, sp_affine_aln* __restrict__ out,
                                                         int t_words_max, int32_t* __restrict__ ckpt_all, uint32_t ckpt_per_slot, uint32_t* __restrict__ ring_all,
                                                         uint32_t* __restrict__ ops_out, uint64_t ops_cap, unsigned long long* __restrict__ cursor, uint64_t* __restrict__ op_off,
                                                         uint32_t* __restrict__ n_cigar) {
    extern __shared__ uint32_t lds[];
    constexpr int BAND = 64 * DPL;
    constexpr int ROWS = DPL == 1 ? AF_MAP_ROWS : AF_MAP_ROWS_WIDE;
    constexpr bool hasn = HASN;
    const int lane = threadIdx.x;
    int32_t* ckpt = ckpt_all + (size_t)blockIdx.x * ckpt_per_slot * (3 * BAND);
    uint32_t* ring = ring_all + (size_t)blockIdx.x * AF_MAP_RING;
    uint32_t* LT = lds; uint32_t* LQ = LT + t_words_max; uint32_t* NT = LQ + t_words_max + 2 * BAND / 16 + 8; uint32_t* NQ = NT + t_words_max;
    uint8_t* tile = (uint8_t*)(NQ + t_words_max + 2 * BAND / 16 + 8);
    const int q1 = o.q, e1 = o.e, q2 = o.q2, e2 = o.e2;
    uint32_t n_run = n_pairs;
    if (n_live) { const uint32_t v = *n_live; n_run = v < n_pairs ? v : n_pairs; }
    for (uint32_t k = blockIdx.x; k < n_run; k += gridDim.x) {
        const uint32_t p = list ? list[k] : k;
        const AfPair pr = pairs[p];
        const int tlen = pr.pad < 0 ? 0 : B.len[pr.b], qlen = pr.pad < 0 ? 0 : A.len[pr.a];
        sp_affine_aln res; res.score = 0; res.nm = 0; res.a_start = res.a_end = res.b_start = res.b_end = 0;
        const int klo = -pr.diag - BAND / 2;
        int i_lo = -(klo + BAND - 1); if (i_lo < 0) i_lo = 0;
        int i_hi = qlen - 1 - klo; if (i_hi > tlen - 1) i_hi = tlen - 1;
        if (pr.pad < 0 || tlen <= 0 || qlen <= 0 || i_lo > i_hi) { if (lane == 0) { out[p] = res; n_cigar[p] = 0; op_off[p] = AF_MAP_NO_OPS; } continue; }
        const int tw0 = i_lo >> 4, tw1 = (i_hi >> 4) + 1;
        int q_lo = i_lo + klo; if (q_lo < 0) q_lo = 0;
        int q_hi = i_hi + klo + BAND - 1; if (q_hi > qlen - 1) q_hi = qlen - 1;
        const int qw0 = q_lo >> 4, qw1 = (q_hi >> 4) + 1;
        spw::wave_lds_sync();                               // (the pair before this one has been read)
        {
            const uint32_t* tw = B.words + B.word_off[pr.b]; const uint32_t* qw = A.words + A.word_off[pr.a];
            const uint32_t* tn = B.nplane ? B.nplane + B.word_off[pr.b] : nullptr; const uint32_t* qn = A.nplane ? A.nplane + A.word_off[pr.a] : nullptr;
            for (int w = lane; w < tw1 - tw0; w += SP_WAVE) { LT[w] = tw[tw0 + w]; if (hasn) NT[w] = tn ? tn[tw0 + w] : 0u; }
            for (int w = lane; w < qw1 - qw0; w += SP_WAVE) { LQ[w] = qw[qw0 + w]; if (hasn) NQ[w] = qn ? qn[qw0 + w] : 0u; }
        }
        spw::wave_lds_sync();
        auto base_of = [&](const uint32_t* W, const uint32_t* N, int pos, int w0) {
            const int w = (pos >> 4) - w0; const uint32_t sh = (uint32_t)(pos & 15) << 1;
            if (hasn && ((N[w] >> sh) & 1u)) return 4;
            return (int)((W[w] >> sh) & 3u);
        };
        // ---- forward: affine_tb_kernel's rows on scores alone (its comparisons, so its decisions): the best cell and the checkpoints
        int hs[DPL], e1s[DPL], e2s[DPL];
#pragma unroll
        for (int c = 0; c < DPL; ++c) hs[c] = e1s[c] = e2s[c] = AF_NEG;
        int bs = 0, bi = -1, bj = -1;
        for (int i = i_lo; i <= i_hi; ++i) {
            if (((i - i_lo) & (ROWS - 1)) == 0) {
                // a lane's DPL scores are DPL consecutive words of each of the checkpoint's three planes
                int32_t* cp = ckpt + (size_t)((i - i_lo) / ROWS) * (3 * BAND) + lane * DPL;
#pragma unroll
                for (int c = 0; c < DPL; ++c) { cp[c] = hs[c]; cp[BAND + c] = e1s[c]; cp[2 * BAND + c] = e2s[c]; }
            }
            const int ct = base_of(LT, NT, i, tw0);
            // the diagonal above the lane's last cell: lane l + 1's first cell of the row before
            const int upH = spw::from_upper(hs[0], AF_NEG), upE1 = spw::from_upper(e1s[0], AF_NEG), upE2 = spw::from_upper(e2s[0], AF_NEG);
            int hA[DPL], a1n[DPL], a2n[DPL]; uint32_t k1[DPL], k2[DPL]; bool valid[DPL];
#pragma unroll
            for (int c = 0; c < DPL; ++c) {
                const int idx = lane * DPL + c, j = i + klo + idx;
                valid[c] = (unsigned)j < (unsigned)qlen;
                const int hus = c + 1 < DPL ? hs[c + 1] : upH, eus = c + 1 < DPL ? e1s[c + 1] : upE1, eu2s = c + 1 < DPL ? e2s[c + 1] : upE2;
                int a1s, a2s;
                { const int eo = hus - q1; a1s = (eus > eo ? eus : eo) - e1; }
                { const int eo = hus - q2; a2s = (eu2s > eo ? eu2s : eo) - e2; }
                if (a1s < AF_NEG) a1s = AF_NEG;
                if (a2s < AF_NEG) a2s = AF_NEG;
                int h = hs[c];
                const int cq = valid[c] ? base_of(LQ, NQ, j, qw0) : 4;
                const bool ambi = ct > 3 || cq > 3;
                const int sub = ambi ? -o.sc_ambi : (ct == cq ? o.a : -o.b);
                if (h <= 0) h = 0;
                h += sub;
                if (a1s > h) h = a1s;
                if (!valid[c]) { h = AF_NEG; a1s = AF_NEG; a2s = AF_NEG; }
                int srcs = h; if (a2s > srcs) srcs = a2s;
                const bool offer = valid[c] && srcs > 0;
                // the scan's keys order by (score + position * e, position): the maximum alone is needed, the counters of AfKey do not ride along
                k1[c] = offer ? (((uint32_t)(srcs + idx * e1) + AF_BIAS) << 8 | (uint32_t)idx) : 0u;
                k2[c] = offer ? (((uint32_t)(srcs + idx * e2) + AF_BIAS) << 8 | (uint32_t)idx) : 0u;
                hA[c] = h; a1n[c] = a1s; a2n[c] = a2s;
            }
            // exclusive prefix maxima over the diagonals to the left: across the lanes by DPP on the lane's maximum, inside a lane cell by cell
            uint32_t in1 = k1[0], in2 = k2[0];
#pragma unroll
            for (int c = 1; c < DPL; ++c) { in1 = af_map_max(in1, k1[c]); in2 = af_map_max(in2, k2[c]); }
            in1 = (uint32_t)spw::from_lower((int)af_map_scan(in1), 0); in2 = (uint32_t)spw::from_lower((int)af_map_scan(in2), 0);
#pragma unroll
            for (int c = 0; c < DPL; ++c) {
                const int idx = lane * DPL + c, j = i + klo + idx;
                int f1s = AF_NEG, f2s = AF_NEG;
                if (in1) f1s = (int)((in1 >> 8) - AF_BIAS) - q1 - idx * e1;
                if (in2) f2s = (int)((in2 >> 8) - AF_BIAS) - q2 - idx * e2;
                int h = hA[c];
                if (valid[c]) {
                    if (f1s > h) h = f1s;
                    if (a2n[c] > h) h = a2n[c];
                    if (f2s > h) h = f2s;
                    if (h <= 0) h = 0;
                    const bool better = h > bs || (h == bs && h > 0 && (i + j < bi + bj || (i + j == bi + bj && i < bi)));
                    bs = better ? h : bs; bi = better ? i : bi; bj = better ? j : bj;
                }
                hs[c] = h; e1s[c] = a1n[c]; e2s[c] = a2n[c];
                in1 = af_map_max(in1, k1[c]); in2 = af_map_max(in2, k2[c]);
            }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const int os = __shfl_xor(bs, d), oi = __shfl_xor(bi, d), oj = __shfl_xor(bj, d);
            if (os > bs || (os == bs && os > 0 && (oi + oj < bi + bj || (oi + oj == bi + bj && oi < bi)))) { bs = os; bi = oi; bj = oj; }
        }
        if (bs <= 0) { if (lane == 0) { out[p] = res; n_cigar[p] = 0; op_off[p] = AF_MAP_NO_OPS; } continue; }
        // ---- the walk back, block by block
        int ci = bi, cidx = bj - bi - klo, st = 0, done = 0;
        uint32_t n_ops = 0, run_op = 0xF, run_len = 0, nm = 0; int si = 0, sj = 0;      // (nm and the start cell are the path's own: the columns that are not '=', the cell the walk ends in)
        auto emit = [&](uint32_t op) {
            nm += (op == 8u || op == 1u || op == 2u) ? 1u : 0u;
            if (op == run_op) { ++run_len; return; }
            if (run_len) { ring[n_ops % AF_MAP_RING] = run_len << 4 | run_op; ++n_ops; }
            run_op = op; run_len = 1;
        };
        while (!done) {
            const int blk = (ci - i_lo) / ROWS, r0 = blk * ROWS, r1 = ci - i_lo;
            spw::wave_lds_sync();                           // (the tile before this one has been read)
            {
                // the block's rows again from its checkpoint: scores alone, affine_tb_kernel's comparisons and records
                const int32_t* cp = ckpt + (size_t)blk * (3 * BAND) + lane * DPL;
                int hs[DPL], e1s[DPL], e2s[DPL];
#pragma unroll
                for (int c = 0; c < DPL; ++c) { hs[c] = cp[c]; e1s[c] = cp[BAND + c]; e2s[c] = cp[2 * BAND + c]; }
                for (int r = r0; r <= r1; ++r) {
                    const int i = i_lo + r;
                    const int ct = base_of(LT, NT, i, tw0);
                    const int upH = spw::from_upper(hs[0], AF_NEG), upE1 = spw::from_upper(e1s[0], AF_NEG), upE2 = spw::from_upper(e2s[0], AF_NEG);
                    int hA[DPL], a1n[DPL], a2n[DPL]; uint32_t k1[DPL], k2[DPL], dir[DPL]; bool valid[DPL];
#pragma unroll
                    for (int c = 0; c < DPL; ++c) {
                        const int idx = lane * DPL + c, j = i + klo + idx;
                        valid[c] = (unsigned)j < (unsigned)qlen;
                        const int hus = c + 1 < DPL ? hs[c + 1] : upH, eus = c + 1 < DPL ? e1s[c + 1] : upE1, eu2s = c + 1 < DPL ? e2s[c + 1] : upE2;
                        int a1s, a2s; uint32_t d = AF_D_DIAG;
                        { const int eo = hus - q1; if (eus > eo) { a1s = eus - e1; d |= AF_D_E1C; } else a1s = eo - e1; }
                        { const int eo = hus - q2; if (eu2s > eo) { a2s = eu2s - e2; d |= AF_D_E2C; } else a2s = eo - e2; }
                        if (a1s < AF_NEG) a1s = AF_NEG;
                        if (a2s < AF_NEG) a2s = AF_NEG;
                        int h = hs[c];
                        const int cq = valid[c] ? base_of(LQ, NQ, j, qw0) : 4;
                        const bool ambi = ct > 3 || cq > 3;
                        const int sub = ambi ? -o.sc_ambi : (ct == cq ? o.a : -o.b);
                        if (h <= 0) { h = 0; d |= AF_D_START; }
                        h += sub;
                        if (ambi || ct != cq) d |= AF_D_X;
                        if (a1s > h) { h = a1s; d = (d & ~7u) | AF_D_E1; }
                        if (!valid[c]) { h = AF_NEG; a1s = AF_NEG; a2s = AF_NEG; }
                        int srcs = h; if (a2s > srcs) srcs = a2s;
                        const bool offer = valid[c] && srcs > 0;
                        k1[c] = offer ? (((uint32_t)(srcs + idx * e1) + AF_BIAS) << 8 | (uint32_t)idx) : 0u;
                        k2[c] = offer ? (((uint32_t)(srcs + idx * e2) + AF_BIAS) << 8 | (uint32_t)idx) : 0u;
                        hA[c] = h; a1n[c] = a1s; a2n[c] = a2s; dir[c] = d;
                    }
                    uint32_t in1 = k1[0], in2 = k2[0];
#pragma unroll
                    for (int c = 1; c < DPL; ++c) { in1 = af_map_max(in1, k1[c]); in2 = af_map_max(in2, k2[c]); }
                    in1 = (uint32_t)spw::from_lower((int)af_map_scan(in1), 0); in2 = (uint32_t)spw::from_lower((int)af_map_scan(in2), 0);
                    uint32_t packed = 0;
#pragma unroll
                    for (int c = 0; c < DPL; ++c) {
                        const int idx = lane * DPL + c;
                        int f1s = AF_NEG, f2s = AF_NEG; uint32_t d = dir[c];
                        if (in1) { const int src_idx = (int)(in1 & 0xFFu), v = (int)((in1 >> 8) - AF_BIAS); f1s = v - q1 - idx * e1; if (src_idx < idx - 1) d |= AF_D_F1C; }
                        if (in2) { const int src_idx = (int)(in2 & 0xFFu), v = (int)((in2 >> 8) - AF_BIAS); f2s = v - q2 - idx * e2; if (src_idx < idx - 1) d |= AF_D_F2C; }
                        int h = hA[c];
                        if (valid[c]) {
                            if (f1s > h) { h = f1s; d = (d & ~7u) | AF_D_F1; }
                            if (a2n[c] > h) { h = a2n[c]; d = (d & ~7u) | AF_D_E2; }
                            if (f2s > h) { h = f2s; d = (d & ~7u) | AF_D_F2; }
                            if (h <= 0) { h = 0; d = (d & ~7u) | AF_D_NONE; }
                        } else d = AF_D_NONE;
                        hs[c] = h; e1s[c] = a1n[c]; e2s[c] = a2n[c];
                        in1 = af_map_max(in1, k1[c]); in2 = af_map_max(in2, k2[c]);
                        packed |= d << (8 * c);
                    }
                    // the row's records: the lane's DPL cells are DPL consecutive bytes of the tile's row -- one byte, or one 32-bit word, a lane
                    if (DPL == 1) tile[(r - r0) * BAND + lane] = (uint8_t)packed;
                    else ((uint32_t*)tile)[(r - r0) * (BAND / 4) + lane] = packed;
                }
            }
            spw::wave_lds_sync();
            if (lane == 0) {
                while (true) {
                    const int r = ci - i_lo - r0;
                    if (r < 0) break;                       // the block before this one
                    if ((unsigned)cidx >= (unsigned)BAND) { done = 2; break; }
                    const uint32_t d = tile[r * BAND + cidx];
                    if (st == 0) {
                        const uint32_t h = d & 7u;
                        if (h == AF_D_DIAG || h == AF_D_START) { emit((d & AF_D_X) ? 8u : 7u); if (h == AF_D_START) { si = ci; sj = ci + klo + cidx; } --ci; if (h == AF_D_START) { done = 1; break; } continue; }
                        if (h >= AF_D_NONE) { done = 2; break; }
                        st = (int)h;
                    }
                    if (st == (int)AF_D_E1 || st == (int)AF_D_E2) {
                        emit(2u); const bool cont = d & (st == (int)AF_D_E1 ? AF_D_E1C : AF_D_E2C); --ci; ++cidx; if (!cont) st = 0;
                    } else {
                        emit(1u); const bool cont = d & (st == (int)AF_D_F1 ? AF_D_F1C : AF_D_F2C); --cidx; if (!cont) st = 0;
                    }
                }
            }
            ci = __shfl(ci, 0); done = __shfl(done, 0);
            if (ci < i_lo && !done) done = 2;
        }
        if (lane == 0) {
            emit(0xE);                                      // closes the last run
            res.score = bs; res.nm = (int32_t)nm; res.b_start = si; res.b_end = bi + 1; res.a_start = sj; res.a_end = bj + 1;
            out[p] = res;
            if (done != 1) { n_cigar[p] = AF_TB_LOST; op_off[p] = AF_MAP_NO_OPS; }
            else {
                n_cigar[p] = n_ops;
                uint64_t at = AF_MAP_NO_OPS;
                if (n_ops <= AF_MAP_RING) {
                    at = atomicAdd(cursor, (unsigned long long)n_ops);
                    if (at + n_ops <= ops_cap) for (uint32_t x = 0; x < n_ops; ++x) ops_out[at + x] = ring[n_ops - 1 - x];
                    else at = AF_MAP_NO_OPS;
                }
                op_off[p] = at;
            }
        }
    }
}

} // namespace

// the K2 map over a device pair list (AfPair rows; pad < 0: no mapping): results, op counts and op offsets per pair, the ops in d_ops (ops_cap words) from *d_cursor on.
// Everything it needs beside them is pooled and sized by the grid, not by the pairs (the two bands keep checkpoint lists of their own: their slots differ in size and number).
int sp_launch_affine_map(sp_ctx* ctx, const sp_seqset* A, const sp_seqset* B, const void* d_pairs, uint64_t n_pairs, const sp_affine_opts& o, int band, sp_affine_aln* d_out,
                         uint32_t* d_n_cigar, uint64_t* d_op_off, uint32_t* d_ops, uint64_t ops_cap, unsigned long long* d_cursor, const char* prof_name,
                         const uint32_t* d_n_live, const uint32_t* d_list, uint64_t prof_cells) {
    if (n_pairs == 0) return SP_OK;
    if (band != 64 && band != 256) return sp_fail(ctx, SP_ERR_INVALID_ARG, "affine map: band must be 64 or 256");
    if (n_pairs > 0xFFFFFFFFull) return sp_fail(ctx, SP_ERR_INVALID_ARG, "affine map: too many pairs");
    if (B->max_len > 65535 || A->max_len > 65535) return sp_fail(ctx, SP_ERR_TOO_LONG, "affine: sequences of up to 65,535 bases");
    const bool wide = band == 256;
    const int rows = wide ? AF_MAP_ROWS_WIDE : AF_MAP_ROWS;
    const uint64_t slots = (uint64_t)ctx->num_cus * (wide ? AF_MAP_SLOTS_WIDE : AF_MAP_SLOTS);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(n_pairs, slots);
    const uint32_t ckpt_per_slot = (uint32_t)(B->max_len / rows + 2);
    int32_t* d_ckpt = (int32_t*)sp_pool(ctx, wide ? "af_map_ckpt_wide" : "af_map_ckpt", (size_t)slots * ckpt_per_slot * 3 * band * 4);
    uint32_t* d_ring = (uint32_t*)sp_pool(ctx, "af_map_ring", (size_t)ctx->num_cus * AF_MAP_SLOTS * AF_MAP_RING * 4);
    if (!d_ckpt || !d_ring) return sp_fail(ctx, SP_ERR_OUT_OF_MEMORY, "affine map buffers");
    const int t_words_max = (B->max_len >> 4) + 4;
    const size_t lds_bytes = sizeof(uint32_t) * (size_t)(4 * t_words_max + 2 * (2 * band / 16 + 8)) + (size_t)rows * band;
    if (lds_bytes > 160 * 1024) return sp_fail(ctx, SP_ERR_TOO_LONG, "affine map: sequences do not fit the LDS");
    const bool hasn = A->has_n || B->has_n;
    ProfScope ps(ctx, prof_name, prof_cells == ~0ull ? n_pairs : prof_cells);
#define SP_AF_MAP_LAUNCH(D, N) do { \
        (void)hipFuncSetAttribute((const void*)affine_map_kernel<D, N>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes); \
        hipLaunchKernelGGL((affine_map_kernel<D, N>), dim3(grid), dim3(64), lds_bytes, ctx->stream, A->view(), B->view(), (const AfPair*)d_pairs, (uint32_t)n_pairs, d_n_live, d_list, o, d_out, t_words_max, \
                           d_ckpt, ckpt_per_slot, d_ring, d_ops, ops_cap, d_cursor, d_op_off, d_n_cigar); } while (0)
    if (wide) { if (hasn) SP_AF_MAP_LAUNCH(4, true); else SP_AF_MAP_LAUNCH(4, false); }
    else { if (hasn) SP_AF_MAP_LAUNCH(1, true); else SP_AF_MAP_LAUNCH(1, false); }
#undef SP_AF_MAP_LAUNCH
    if (hipGetLastError() != hipSuccess) return sp_fail(ctx, SP_ERR_HIP, "affine map launch failed");
    return SP_OK;
}

// sp_variant.hip -- K6: variant-gene diplotype search on gfx950 (src/diplotyper.rs:1211-1509,
// src/data_types/normalized_variant.rs:431-479).  Pure integer set logic: one thread per
// (het assignment, haplotype side, database haplotype) cell, scores packed into one u64 so the lexicographic
// (core missing, core extra, sub missing, sub extra) order is an integer order.
#include "sp_internal.h"
#include "sp_json.h"
#include <system_error>
#include <thread>
#include <atomic>
#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#define K6_MAX_OBS   64
#define K6_MAX_SLOTS 64
#define K6_NOKEY     0xFFFFFFFFFFFFFFFFull

// quant_match + core/sub split for one (observed subset, haplotype) cell.
//   match_slot[h][o] : first slot of haplotype h that lists observed variant o, or -1   (normalized_variant.rs:443-447)
// The problems of a batch (a panel, one GPU's share of a cohort: 18-23 genes x 32 samples) are ONE launch: their tables lie back to back, a
// thread finds its problem by a binary search over the problems' first cells.
struct K6Desc { int n_haps, n_obs, n_sides, pad; unsigned long long n_comb, cell_base; uint32_t off_ms, off_h, off_o, pad2; };

// The score of one cell -- side `side` of het assignment `comb` against haplotype h -- as one integer.  k6_cells_kernel (the solve) and k6_alt_kernel (the
// alternatives pass) both call it on the same uploaded tables: a cell's key is the same bits wherever it is computed.
__device__ __forceinline__ unsigned long long k6_cell_key(int h, int side, unsigned long long comb, int n_obs, const signed char* __restrict__ match_slot,
                                                          const unsigned long long* __restrict__ slot_need, const unsigned long long* __restrict__ slot_core,
                                                          const unsigned char* __restrict__ obs_core, const unsigned char* __restrict__ obs_het,
                                                          const unsigned char* __restrict__ obs_group, const unsigned char* __restrict__ obs_orient01) {
    unsigned long long matched = 0;
    unsigned ev_core = 0, ev_sub = 0;
    // a side's list is the homozygous variants first (base_haplotype, diplotyper.rs:1219-1222,1269-1270) and then the heterozygous ones that
    // go to it, each in call order: when two of them compete for one slot (alternatives of an OR-group), the one that comes first takes it
    for (int pass = 0; pass < 2; ++pass)
        for (int o = 0; o < n_obs; ++o) {
            if ((obs_het[o] != 0) != (pass == 1)) continue;
            bool in_set = true;
            if (obs_het[o]) {                                                    // het assignment (diplotyper.rs:1270-1317)
                const bool is_h1 = ((comb >> obs_group[o]) & 1ull) != 0;
                const bool to_h1 = is_h1 == (obs_orient01[o] != 0);
                in_set = side == 0 ? to_h1 : !to_h1;
            }
            if (!in_set) continue;
            const int mi = match_slot[(size_t)h * n_obs + o];
            if (mi >= 0 && !((matched >> mi) & 1ull)) matched |= 1ull << mi;
            else { if (obs_core[o]) ++ev_core; else ++ev_sub; }
        }
    const unsigned long long missing = slot_need[h] & ~matched;                   // unmatched slots without a None alternative
    const unsigned mv_core = (unsigned)__popcll(missing & slot_core[h]), mv_sub = (unsigned)__popcll(missing & ~slot_core[h]);
    return ((unsigned long long)mv_core << 48) | ((unsigned long long)ev_core << 32) | ((unsigned long long)mv_sub << 16) | (unsigned long long)ev_sub;
}

__global__ __launch_bounds__(256) void k6_cells_kernel(uint32_t n_prob, unsigned long long total, const K6Desc* __restrict__ desc,
                                                       const signed char* __restrict__ match_slot_all, const unsigned long long* __restrict__ slot_need_all,
                                                       const unsigned long long* __restrict__ slot_core_all, const unsigned char* __restrict__ hap_skip_all,
                                                       const unsigned char* __restrict__ obs_core_all, const unsigned char* __restrict__ obs_het_all,
                                                       const unsigned char* __restrict__ obs_group_all, const unsigned char* __restrict__ obs_orient_all,
                                                       unsigned long long* __restrict__ keys /* per problem [comb][side][hap], problems back to back */) {
    const unsigned long long gcell = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gcell >= total) return;
    uint32_t lo = 0, hi = n_prob;                                    // last problem whose first cell is <= gcell
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (desc[mid].cell_base <= gcell) lo = mid; else hi = mid; }
    const K6Desc D = desc[lo];
    const int n_haps = D.n_haps, n_sides = D.n_sides;
    const unsigned long long cell = gcell - D.cell_base;
    const int h = (int)(cell % (unsigned long long)n_haps);
    const unsigned long long cs = cell / (unsigned long long)n_haps;
    const int side = (int)(cs % (unsigned long long)n_sides);
    const unsigned long long comb = cs / (unsigned long long)n_sides;
    if (hap_skip_all[D.off_h + h]) { keys[gcell] = K6_NOKEY; return; }        // SV haplotypes are not quantified (:1443-1446)
    keys[gcell] = k6_cell_key(h, side, comb, D.n_obs, match_slot_all + D.off_ms, slot_need_all + D.off_h, slot_core_all + D.off_h,
                              obs_core_all + D.off_o, obs_het_all + D.off_o, obs_group_all + D.off_o, obs_orient_all + D.off_o);
}

// ---------------------------------------------------------------- the alternatives pass (sp_variant_alternatives; the definition: include/starphase_hip.h)
// One wave per workgroup.  A problem owns wg_count consecutive workgroups (the host hands the CUs' worth of workgroups out over the problems of the
// batch); workgroup w of a problem takes the assignments w, w + wg_count, ... and keeps the N best candidates it has met in LDS.  Nothing of size
// n_comb x n_haps exists anywhere: a cell's key lives in a register until the sorted N-entry list of its side has taken or refused it.
//
// Why a side's N smallest (key, h) are enough: take a candidate (comb, h0, h1) whose h1 is not among the N smallest of side 1.  The N candidates
// (comb, h0, h') with h' from those N have key' + key0 <= key1 + key0, the same comb and dip0, and (key', h') < (key1, h1): N candidates precede it,
// so it is none of the N best.  The same holds for side 0, so the N x N sums hold every candidate of the assignment that can be listed.
//
// The lists are kept by ranking, not by N rounds of a minimum: a tile of up to 64 new items and the sorted list are merged by giving every item its
// rank in the union (the order is strict, so the ranks are a permutation) and storing those below N at their rank.  A tile none of whose items beats the
// list's last entry is dropped after one ballot; that test only skips work, the list is the same without it.
#define K6_ALT_MAXN 64
#define K6_LOW48    0xFFFFFFFFFFFFull
struct K6AltDesc { int n_haps, n_obs, n_sides, pad; unsigned long long n_comb; uint32_t wg_base, wg_count, off_ms, off_h, off_o, pad2; };
struct K6Side { unsigned long long key; int h, pad; };                                                       // ordered by (key, h); h < 0: an SV label
struct K6Cand { unsigned long long total, key0, key1; uint32_t comb; int dip0, dip1; uint32_t kept; };       // ordered by (total, comb, dip0, dip1)
struct K6Part { unsigned long long n_cand, best, n_kept; uint32_t n_rec, pad; };                             // what one workgroup hands to the selection

__device__ __forceinline__ bool k6_less(const K6Side& a, const K6Side& b) { return a.key != b.key ? a.key < b.key : a.h < b.h; }
__device__ __forceinline__ bool k6_less(const K6Cand& a, const K6Cand& b) {
    if (a.total != b.total) return a.total < b.total;
    if (a.comb != b.comb) return a.comb < b.comb;
    if (a.dip0 != b.dip0) return a.dip0 < b.dip0;
    return a.dip1 < b.dip1;
}
__device__ __forceinline__ unsigned long long k6_wave_min(unsigned long long v) {
    for (int m = 32; m > 0; m >>= 1) { const unsigned long long o = __shfl_xor(v, m, 64); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ unsigned long long k6_wave_sum(unsigned long long v) {
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// cur[0 .. n) sorted, one new item per lane (valid) -> cur holds the N smallest of both, sorted; n grows.  Called by all 64 lanes of the one wave.
template <class T>
__device__ void k6_merge(T* cur, T* nxt, T* tile, int& n, bool valid, const T& it, int N) {
    const int lane = (int)threadIdx.x;
    const bool want = valid && (n < N || k6_less(it, cur[N - 1]));
    const unsigned long long m = __ballot(want);
    if (!m) return;
    if (want) tile[lane] = it;
    __syncthreads();
    if (want) {
        int r = 0;
        for (int k = 0; k < n; ++k) r += k6_less(cur[k], it) ? 1 : 0;
        for (unsigned long long mm = m; mm; mm &= mm - 1) { const int t = __ffsll((long long)mm) - 1; if (t != lane) r += k6_less(tile[t], it) ? 1 : 0; }
        if (r < N) nxt[r] = it;
    }
    if (lane < n) {
        const T c = cur[lane];
        int r = lane;
        for (unsigned long long mm = m; mm; mm &= mm - 1) { const int t = __ffsll((long long)mm) - 1; r += k6_less(tile[t], c) ? 1 : 0; }
        if (r < N) nxt[r] = c;
    }
    __syncthreads();
    n = min(N, n + (int)__popcll(m));
    if (lane < n) cur[lane] = nxt[lane];
    __syncthreads();
}

// Both kernels of the pass are launched with 64 threads and nothing else: a workgroup is ONE wave.  k6_merge's ballot, the wave reductions and "lane < N covers the
// list" all rest on that; the barriers order the wave's own LDS traffic (they cost a single wave next to nothing), they do not join several waves.
__global__ __launch_bounds__(64) void k6_alt_kernel(uint32_t n_prob, int N, const K6AltDesc* __restrict__ desc,
                                                    const signed char* __restrict__ match_slot_all, const unsigned long long* __restrict__ slot_need_all,
                                                    const unsigned long long* __restrict__ slot_core_all, const unsigned char* __restrict__ hap_skip_all,
                                                    const unsigned char* __restrict__ hap_core_all, const unsigned char* __restrict__ obs_core_all,
                                                    const unsigned char* __restrict__ obs_het_all, const unsigned char* __restrict__ obs_group_all,
                                                    const unsigned char* __restrict__ obs_orient_all, const int* __restrict__ obs_sv_all,
                                                    const unsigned char* __restrict__ obs_svd_all /* the labels of a problem numbered 0 .. 63, 0xFF: none */,
                                                    K6Cand* __restrict__ part_rec /* [workgroup][N] */, K6Part* __restrict__ part) {
    __shared__ K6Side s_cur[2][K6_ALT_MAXN], s_nxt[K6_ALT_MAXN], s_tile[64];
    __shared__ K6Cand c_cur[K6_ALT_MAXN], c_nxt[K6_ALT_MAXN], c_tile[64];
    const int lane = (int)threadIdx.x;
    const uint32_t wg = blockIdx.x;
    uint32_t lo = 0, hi = n_prob;                                    // last problem whose first workgroup is <= wg
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (desc[mid].wg_base <= wg) lo = mid; else hi = mid; }
    const K6AltDesc D = desc[lo];
    const int H = D.n_haps, n_obs = D.n_obs, n_sides = D.n_sides;
    const signed char* match_slot = match_slot_all + D.off_ms;
    const unsigned long long* slot_need = slot_need_all + D.off_h; const unsigned long long* slot_core = slot_core_all + D.off_h;
    const unsigned char* hap_skip = hap_skip_all + D.off_h; const unsigned char* hap_core = hap_core_all + D.off_h;
    const unsigned char* obs_core = obs_core_all + D.off_o; const unsigned char* obs_het = obs_het_all + D.off_o;
    const unsigned char* obs_group = obs_group_all + D.off_o; const unsigned char* obs_orient01 = obs_orient_all + D.off_o;
    const int* obs_sv = obs_sv_all + D.off_o; const unsigned char* obs_svd = obs_svd_all + D.off_o;
    int n_run = 0;
    unsigned long long n_cand = 0, w_best = K6_NOKEY, w_kept = 0;
    for (unsigned long long comb = wg - D.wg_base; comb < D.n_comb; comb += D.wg_count) {
        __syncthreads();                                                         // the side lists of the assignment before have been read (a k6_merge that drops its tile returns without a barrier)
        int ns[2] = {0, 0};
        unsigned long long elig[2] = {0, 0}, sbest[2] = {0, 0}, kept[2] = {0, 0};
        bool anysub[2] = {false, false}, sv[2] = {false, false};
        for (int side = 0; side < n_sides; ++side) {
            // the SV short-circuit (:1414-1431): the first label of the side's members explains it, the distinct labels behind it are unexpected core variants
            int first = -1; unsigned long long rest = 0;
            for (int pass = 0; pass < 2; ++pass)
                for (int o = 0; o < n_obs; ++o) {
                    if ((obs_het[o] != 0) != (pass == 1) || obs_sv[o] < 0) continue;
                    if (obs_het[o]) {
                        const bool is_h1 = ((comb >> obs_group[o]) & 1ull) != 0;
                        const bool to_h1 = is_h1 == (obs_orient01[o] != 0);
                        if ((side == 0) != to_h1) continue;
                    }
                    if (first < 0) first = obs_sv[o]; else rest |= 1ull << (obs_svd[o] & 63);
                }
            int n = 0;
            if (first >= 0) {
                sv[side] = true; elig[side] = 1; kept[side] = 1; sbest[side] = (unsigned long long)__popcll(rest) << 32;
                if (lane == 0) { K6Side e; e.key = sbest[side]; e.h = -(first + 2); e.pad = 0; s_cur[side][0] = e; }
                __syncthreads();
                n = 1;
            } else {
                unsigned long long l_best = K6_NOKEY, l_sub = 0, l_core = 0, e_all = 0;
                for (int base = 0; base < H; base += 64) {
                    const int h = base + lane;
                    bool ok = h < H && !hap_skip[h];
                    K6Side it; it.key = K6_NOKEY; it.h = h; it.pad = 0;
                    if (ok) {
                        it.key = k6_cell_key(h, side, comb, n_obs, match_slot, slot_need, slot_core, obs_core, obs_het, obs_group, obs_orient01);
                        ok = (it.key >> 48) <= 1;                                // the (1, MAX, MAX, MAX) bound of find_best_inexact_matches
                    }
                    e_all += (unsigned long long)__popcll(__ballot(ok));
                    if (ok) {
                        if (it.key < l_best) { l_best = it.key; l_sub = 0; l_core = 0; }
                        if (it.key == l_best) { if (hap_core[h]) ++l_core; else ++l_sub; }
                    }
                    k6_merge(s_cur[side], s_nxt, s_tile, n, ok, it, N);
                }
                elig[side] = e_all;
                if (e_all) {
                    const unsigned long long b = k6_wave_min(l_best);
                    const unsigned long long nsub = k6_wave_sum(l_best == b ? l_sub : 0), ncore = k6_wave_sum(l_best == b ? l_core : 0);
                    sbest[side] = b; anysub[side] = nsub > 0; kept[side] = nsub > 0 ? nsub : ncore;         // sub-alleles shadow core alleles at the side's best key
                }
            }
            ns[side] = n;
        }
        // what solve_diplotype makes of this assignment: the sum of the sides' best scores, (1, MAX, MAX, MAX) for a side nothing explains
        const bool one = n_sides == 1;
        const bool ok_all = elig[0] > 0 && (one || elig[1] > 0);
        unsigned long long a_best, a_kept = 0;
        if (ok_all) { a_best = one ? sbest[0] : sbest[0] + sbest[1]; a_kept = one ? kept[0] : kept[0] * kept[1]; }
        else {
            const unsigned long long cm = (elig[0] ? sbest[0] >> 48 : 1ull) + (one ? 0ull : (elig[1] ? sbest[1] >> 48 : 1ull));
            a_best = (cm << 48) | K6_LOW48;
        }
        if (a_best < w_best) { w_best = a_best; w_kept = a_kept; } else if (a_best == w_best) w_kept += a_kept;
        if (!ok_all) continue;
        n_cand += one ? elig[0] : elig[0] * elig[1];
        if (n_run == N && a_best > c_cur[N - 1].total) continue;                   // even the assignment's best total comes behind the N kept
        const int n1 = one ? 1 : ns[1];
        const int n_pairs = one ? ns[0] : ns[0] * ns[1];
        for (int pb = 0; pb < n_pairs; pb += 64) {
            const int p = pb + lane;
            const bool valid = p < n_pairs;
            K6Cand c; c.total = 0; c.key0 = 0; c.key1 = 0; c.comb = (uint32_t)comb; c.dip0 = 0; c.dip1 = 0; c.kept = 0;
            if (valid) {
                const K6Side a = s_cur[0][one ? p : p / n1];
                const K6Side b = one ? a : s_cur[1][p % n1];
                c.key0 = a.key; c.key1 = b.key; c.total = one ? a.key : a.key + b.key; c.dip0 = a.h; c.dip1 = b.h;
                const bool k0 = sv[0] || (a.key == sbest[0] && !(anysub[0] && hap_core[a.h]));
                const bool k1 = one ? k0 : (sv[1] || (b.key == sbest[1] && !(anysub[1] && hap_core[b.h])));
                c.kept = (k0 && k1) ? 1u : 0u;
            }
            k6_merge(c_cur, c_nxt, c_tile, n_run, valid, c, N);
        }
    }
    __syncthreads();
    if (lane < N) {
        K6Cand z; z.total = 0; z.key0 = 0; z.key1 = 0; z.comb = 0; z.dip0 = 0; z.dip1 = 0; z.kept = 0;
        part_rec[(size_t)wg * N + lane] = lane < n_run ? c_cur[lane] : z;
    }
    if (lane == 0) { K6Part P; P.n_cand = n_cand; P.best = w_best; P.n_kept = w_kept; P.n_rec = (uint32_t)n_run; P.pad = 0; part[wg] = P; }
}

// One workgroup per problem: the workgroups' lists merged in workgroup order into the final N, the counters summed, the flags set, the records written
// in the ABI's layout (the unused ones zero).
__global__ __launch_bounds__(64) void k6_alt_select_kernel(int N, const K6AltDesc* __restrict__ desc, const K6Cand* __restrict__ part_rec, const K6Part* __restrict__ part,
                                                           sp_variant_alt* __restrict__ out /* [problem][N] */, sp_variant_alt_info* __restrict__ info) {
    __shared__ K6Cand c_cur[K6_ALT_MAXN], c_nxt[K6_ALT_MAXN], c_tile[64];
    const int lane = (int)threadIdx.x;
    const K6AltDesc D = desc[blockIdx.x];
    int n = 0;
    unsigned long long l_best = K6_NOKEY, l_cand = 0;
    for (uint32_t w = lane; w < D.wg_count; w += 64) { const K6Part P = part[D.wg_base + w]; l_best = P.best < l_best ? P.best : l_best; l_cand += P.n_cand; }
    const unsigned long long best = k6_wave_min(l_best), n_cand = k6_wave_sum(l_cand);
    unsigned long long l_kept = 0;
    for (uint32_t w = lane; w < D.wg_count; w += 64) { const K6Part P = part[D.wg_base + w]; if (P.best == best) l_kept += P.n_kept; }
    const unsigned long long n_kept = k6_wave_sum(l_kept);
    for (uint32_t w = 0; w < D.wg_count; ++w) {
        const uint32_t n_rec = part[D.wg_base + w].n_rec;
        const bool valid = (uint32_t)lane < n_rec;
        K6Cand c; c.total = 0; c.key0 = 0; c.key1 = 0; c.comb = 0; c.dip0 = 0; c.dip1 = 0; c.kept = 0;
        if (valid) c = part_rec[(size_t)(D.wg_base + w) * N + lane];
        k6_merge(c_cur, c_nxt, c_tile, n, valid, c, N);
    }
    __syncthreads();
    if (lane < N) {
        sp_variant_alt a;
        for (int k = 0; k < 4; ++k) { a.score[k] = 0; a.side_score[0][k] = 0; a.side_score[1][k] = 0; }
        a.dip[0] = 0; a.dip[1] = 0; a.comb = 0; a.flags = 0;
        if (lane < n) {
            const K6Cand c = c_cur[lane];
            for (int k = 0; k < 4; ++k) {
                a.score[k] = (int64_t)((c.total >> (48 - 16 * k)) & 0xFFFF);
                a.side_score[0][k] = (int32_t)((c.key0 >> (48 - 16 * k)) & 0xFFFF); a.side_score[1][k] = (int32_t)((c.key1 >> (48 - 16 * k)) & 0xFFFF);
            }
            a.dip[0] = c.dip0; a.dip[1] = c.dip1; a.comb = (int32_t)c.comb;
            a.flags = c.total == best ? (c.kept ? SP_VAR_ALT_CALLED : SP_VAR_ALT_SHADOWED) : 0u;
        }
        out[(size_t)blockIdx.x * N + lane] = a;
    }
    if (lane == 0) {
        sp_variant_alt_info I;
        I.n_comb = D.n_comb; I.n_candidates = n_cand;
        const bool unset = (best & K6_LOW48) == K6_LOW48;                        // an assignment with a side nothing explains: (core missing, MAX, MAX, MAX)
        I.best_score[0] = (int64_t)(best >> 48);
        for (int k = 1; k < 4; ++k) I.best_score[k] = unset ? INT64_MAX : (int64_t)((best >> (48 - 16 * k)) & 0xFFFF);
        I.n_alts = (uint32_t)n; I.n_called = n_kept > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n_kept;
        info[blockIdx.x] = I;
    }
}

namespace {

// the host tables of one problem (what the kernel reads, and what the combination of the sides needs)
struct K6Prep {
    int H = 0, NO = 0, n_sides = 1, n_het = 0;
    unsigned long long n_comb = 1, n_cells = 0;
    std::vector<uint8_t> obs_het, obs_group, obs_orient, obs_core, hap_skip;
    std::vector<int8_t> match_slot;
    std::vector<unsigned long long> slot_need, slot_core;
};

int32_t k6_prep(sp_ctx* ctx, const sp_variant_problem* p, K6Prep& q) {
    const int H = p->n_haps, NO = p->n_obs;
    q.H = H; q.NO = NO;
    if (NO > K6_MAX_OBS) return sp_fail(ctx, SP_ERR_TOO_LONG, "variant solve: more than 64 observed variants");
    // which observed variants are hom / het, het groups in first-seen order (diplotyper.rs:1216-1240,1270-1300)
    q.obs_het.assign(std::max(1, NO), 0); q.obs_group.assign(std::max(1, NO), 0); q.obs_orient.assign(std::max(1, NO), 1); q.obs_core.assign(std::max(1, NO), 1);
    std::vector<std::pair<int64_t, int>> ps_bit;             // phase set -> bit of the het assignment, in first-seen order
    int groups = 0, n_het = 0;
    for (int o = 0; o < NO; ++o) {
        if (p->obs_var[o] < 0 || p->obs_var[o] >= p->n_vars) return sp_fail(ctx, SP_ERR_INVALID_ARG, "variant solve: variant id out of range");
        q.obs_core[o] = p->var_is_core[p->obs_var[o]];
        const int gt = p->obs_gt[o];
        if (gt == SP_GT_HOM_REF) return sp_fail(ctx, SP_ERR_INVALID_ARG, "variant solve: homozygous reference calls must not be passed");
        if (gt == SP_GT_HOM_ALT) continue;
        q.obs_het[o] = 1; ++n_het; q.obs_orient[o] = gt != SP_GT_HET_FLIP;
        int bit = -1;
        if (p->obs_ps[o] >= 0) {
            for (auto& kv : ps_bit) if (kv.first == p->obs_ps[o]) bit = kv.second;
            if (bit < 0) { bit = groups++; ps_bit.emplace_back(p->obs_ps[o], bit); }
        } else bit = groups++;                                  // an unphased het is its own group
        q.obs_group[o] = (uint8_t)bit;
    }
    if (groups > 24) return sp_fail(ctx, SP_ERR_TOO_LONG, "variant solve: more than 24 independent heterozygous groups");
    q.n_het = n_het;
    q.n_comb = n_het ? (1ull << (groups - 1)) : 1ull;
    q.n_sides = n_het ? 2 : 1;
    // per haplotype tables
    q.match_slot.assign((size_t)std::max(1, H) * std::max(1, NO), -1);
    q.slot_need.assign(std::max(1, H), 0); q.slot_core.assign(std::max(1, H), 0); q.hap_skip.assign(std::max(1, H), 0);
    for (int h = 0; h < H; ++h) {
        q.hap_skip[h] = p->hap_is_sv[h] ? 1 : 0;
        const int s0 = p->slot_off[h], s1 = p->slot_off[h + 1];
        if (s1 - s0 > K6_MAX_SLOTS) return sp_fail(ctx, SP_ERR_TOO_LONG, "variant solve: haplotype with more than 64 variants");
        for (int s = s0; s < s1; ++s) {
            bool has_none = false; int first_some = -1;
            for (int x = p->alt_off[s]; x < p->alt_off[s + 1]; ++x) { if (p->alt_var[x] < 0) has_none = true; else if (first_some < 0) first_some = p->alt_var[x]; }
            if (!has_none) q.slot_need[h] |= 1ull << (s - s0);
            if (first_some >= 0 && p->var_is_core[first_some]) q.slot_core[h] |= 1ull << (s - s0);
        }
        for (int o = 0; o < NO; ++o)
            for (int s = s0; s < s1 && q.match_slot[(size_t)h * NO + o] < 0; ++s)
                for (int x = p->alt_off[s]; x < p->alt_off[s + 1]; ++x) if (p->alt_var[x] == p->obs_var[o]) { q.match_slot[(size_t)h * NO + o] = (int8_t)(s - s0); break; }
    }
    q.n_cells = q.n_comb * (unsigned long long)q.n_sides * (unsigned long long)std::max(1, H);
    return SP_OK;
}

// per side: best tuple under the (1, MAX, MAX, MAX) bound, ties, sub-allele shadowing; then the sides of every het assignment (diplotyper.rs:1246-1371,1433-1509)
void k6_combine(const sp_variant_problem* p, const K6Prep& q, const unsigned long long* keys, sp_variant_result* res) {
    const int H = q.H, NO = q.NO, n_sides = q.n_sides;
    // SV short-circuit is decided per side on the host (diplotyper.rs:1414-1431): collect labels of a side
    auto side_members = [&](unsigned long long comb, int side, std::vector<int>& out) {
        out.clear();
        for (int pass = 0; pass < 2; ++pass)                  // the homozygous variants first, then the side's heterozygous ones (diplotyper.rs:1269-1317)
            for (int o = 0; o < NO; ++o) {
                if ((q.obs_het[o] != 0) != (pass == 1)) continue;
                bool in_set = true;
                if (q.obs_het[o]) { const bool is_h1 = ((comb >> q.obs_group[o]) & 1ull) != 0; const bool to_h1 = is_h1 == (q.obs_orient[o] != 0); in_set = side == 0 ? to_h1 : !to_h1; }
                if (in_set) out.push_back(o);
            }
    };
    struct Side { int64_t score[4]; bool is_sv; int sv_label; std::vector<int> best; };
    auto solve_side = [&](unsigned long long comb, int side, Side& out) {
        std::vector<int> mem; side_members(comb, side, mem);
        out.best.clear(); out.is_sv = false; out.sv_label = -1;
        std::vector<int> labels;
        for (int o : mem) if (p->obs_sv_label[o] >= 0) labels.push_back(p->obs_sv_label[o]);
        if (!labels.empty()) {
            std::vector<int> rest(labels.begin() + 1, labels.end());
            std::sort(rest.begin(), rest.end()); rest.erase(std::unique(rest.begin(), rest.end()), rest.end());
            out.is_sv = true; out.sv_label = labels[0];
            out.score[0] = 0; out.score[1] = (int64_t)rest.size(); out.score[2] = 0; out.score[3] = 0;
            return;
        }
        unsigned long long best = K6_NOKEY;
        const unsigned long long* k = keys + (comb * (unsigned long long)n_sides + (unsigned long long)side) * (unsigned long long)std::max(1, H);
        for (int h = 0; h < H; ++h) if (k[h] != K6_NOKEY && (k[h] >> 48) <= 1 && k[h] < best) best = k[h];
        if (best == K6_NOKEY) { out.score[0] = 1; out.score[1] = out.score[2] = out.score[3] = INT64_MAX; return; }
        bool any_sub = false;
        for (int h = 0; h < H; ++h) if (k[h] == best && !p->hap_is_core[h]) any_sub = true;
        for (int h = 0; h < H; ++h) if (k[h] == best && (!p->hap_is_core[h]) == any_sub) out.best.push_back(h);
        out.score[0] = (int64_t)(best >> 48); out.score[1] = (int64_t)((best >> 32) & 0xFFFF); out.score[2] = (int64_t)((best >> 16) & 0xFFFF); out.score[3] = (int64_t)(best & 0xFFFF);
    };
    auto push_pairs = [&](const Side& a, const Side& b, int comb) {
        const size_t na = a.is_sv ? 1 : a.best.size(), nb = b.is_sv ? 1 : b.best.size();
        for (size_t i = 0; i < na; ++i) for (size_t j = 0; j < nb; ++j) {
            if (res->n_dip >= SP_VAR_MAXDIP) { res->overflow = 1; return; }
            res->dip[res->n_dip][0] = a.is_sv ? -(a.sv_label + 2) : a.best[i];
            res->dip[res->n_dip][1] = b.is_sv ? -(b.sv_label + 2) : b.best[j];
            res->dip_comb[res->n_dip] = comb; res->n_dip++;
        }
    };
    if (!q.n_het) {
        Side s; solve_side(0, 0, s);
        for (int k = 0; k < 4; ++k) res->score[k] = s.score[k];
        push_pairs(s, s, 0);
        // a homozygous call pairs every haplotype with itself only (diplotyper.rs:1246-1256)
        int w = 0; for (int i = 0; i < res->n_dip; ++i) if (res->dip[i][0] == res->dip[i][1]) { res->dip[w][0] = res->dip[i][0]; res->dip[w][1] = res->dip[i][1]; res->dip_comb[w] = 0; ++w; }
        res->n_dip = w;
        return;
    }
    int64_t best[4] = {INT64_MAX, INT64_MAX, INT64_MAX, INT64_MAX};
    for (unsigned long long comb = 0; comb < q.n_comb; ++comb) {
        Side a, b; solve_side(comb, 0, a); solve_side(comb, 1, b);
        int64_t tot[4]; int cmp = 0;
        for (int k = 0; k < 4; ++k) tot[k] = (a.score[k] == INT64_MAX || b.score[k] == INT64_MAX) ? INT64_MAX : a.score[k] + b.score[k];
        for (int k = 0; k < 4 && !cmp; ++k) cmp = tot[k] < best[k] ? -1 : (tot[k] > best[k]);
        if (cmp < 0) { std::memcpy(best, tot, sizeof(best)); res->n_dip = 0; }
        if (cmp <= 0) push_pairs(a, b, (int)comb);
    }
    for (int k = 0; k < 4; ++k) res->score[k] = best[k];
}

template <class T> void append(std::vector<uint8_t>& blob, const std::vector<T>& v) { const uint8_t* p = reinterpret_cast<const uint8_t*>(v.data()); blob.insert(blob.end(), p, p + v.size() * sizeof(T)); }

} // namespace

// The solves of a panel or of one GPU's share of a cohort (23 genes x 32 samples) in one launch: the tables of all problems go up in one
// copy, every (het assignment, side, haplotype) cell of every problem is one thread of one kernel, the keys come back in one copy and the
// sides are combined on the host (round 2 ran one launch + one wait per problem on three streams: ~1 ms each).  results[i] / problem_rc[i]
// are what sp_variant_solve gives for problems[i]; a problem that fails its checks is reported in problem_rc and takes no part in the launch.
extern "C" int32_t sp_variant_solve_batch(sp_ctx* ctx, uint32_t n, const sp_variant_problem* const* problems, sp_variant_result* results, int32_t* problem_rc) {
    if (!ctx) return SP_ERR_INVALID_ARG;
    if (n && (!problems || !results)) return sp_fail(ctx, SP_ERR_INVALID_ARG, "sp_variant_solve_batch: null argument");
    for (uint32_t i = 0; i < n; ++i) if (!problems[i]) return sp_fail(ctx, SP_ERR_INVALID_ARG, "sp_variant_solve_batch: null problem");
    if (n == 0) return SP_OK;
    (void)hipSetDevice(ctx->device);
    std::vector<K6Prep> prep(n);
    std::vector<int32_t> rcs(n, SP_OK);
    std::string first_err; int32_t rc = SP_OK;
    std::vector<K6Desc> desc; std::vector<uint32_t> which;
    std::vector<uint8_t> ms, need, core, skip, oc, oh, og, oo;
    unsigned long long total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        std::memset(&results[i], 0, sizeof(results[i]));
        rcs[i] = k6_prep(ctx, problems[i], prep[i]);
        if (rcs[i] != SP_OK) { if (rc == SP_OK) { rc = rcs[i]; first_err = ctx->err; } continue; }
        const K6Prep& q = prep[i];
        if (q.H <= 0) continue;                                   // no haplotypes: every key stays unset, the combination runs on the host alone
        K6Desc d; std::memset(&d, 0, sizeof d);
        d.n_haps = q.H; d.n_obs = q.NO; d.n_sides = q.n_sides; d.n_comb = q.n_comb; d.cell_base = total;
        d.off_ms = (uint32_t)ms.size(); d.off_h = (uint32_t)skip.size(); d.off_o = (uint32_t)oc.size();
        append(ms, q.match_slot); append(need, q.slot_need); append(core, q.slot_core); append(skip, q.hap_skip);
        append(oc, q.obs_core); append(oh, q.obs_het); append(og, q.obs_group); append(oo, q.obs_orient);
        desc.push_back(d); which.push_back(i);
        total += q.n_cells;
    }
    std::vector<unsigned long long> keys;
    if (total > 0) {
        // one staging blob up (pinned), one key array down
        size_t bytes = 0;
        auto place = [&](size_t b) { const size_t at = (bytes + 15) & ~(size_t)15; bytes = at + b; return at; };
        const size_t a_desc = place(desc.size() * sizeof(K6Desc)), a_ms = place(ms.size()), a_need = place(need.size()), a_core = place(core.size()), a_skip = place(skip.size());
        const size_t a_oc = place(oc.size()), a_oh = place(oh.size()), a_og = place(og.size()), a_oo = place(oo.size());
        uint8_t* h_in = (uint8_t*)sp_host_pool(ctx, "k6_in", bytes + 16); uint8_t* d_in = (uint8_t*)sp_pool(ctx, "k6_in", bytes + 16);
        unsigned long long* d_keys = (unsigned long long*)sp_pool(ctx, "k6_keys", total * 8);
        unsigned long long* h_keys = (unsigned long long*)sp_host_pool(ctx, "k6_keys", total * 8);
        if (!h_in || !d_in || !d_keys || !h_keys) return sp_fail(ctx, SP_ERR_OUT_OF_MEMORY, "variant solve buffers");
        std::memcpy(h_in + a_desc, desc.data(), desc.size() * sizeof(K6Desc));
        std::memcpy(h_in + a_ms, ms.data(), ms.size()); std::memcpy(h_in + a_need, need.data(), need.size()); std::memcpy(h_in + a_core, core.data(), core.size());
        std::memcpy(h_in + a_skip, skip.data(), skip.size()); std::memcpy(h_in + a_oc, oc.data(), oc.size()); std::memcpy(h_in + a_oh, oh.data(), oh.size());
        std::memcpy(h_in + a_og, og.data(), og.size()); std::memcpy(h_in + a_oo, oo.data(), oo.size());
        SP_HIP_CHECK(ctx, hipMemcpyAsync(d_in, h_in, bytes, hipMemcpyHostToDevice, ctx->stream));
        {
            ProfScope ps(ctx, "k6_cells", total);
            hipLaunchKernelGGL(k6_cells_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, (uint32_t)desc.size(), total,
                               (const K6Desc*)(d_in + a_desc), (const signed char*)(d_in + a_ms), (const unsigned long long*)(d_in + a_need),
                               (const unsigned long long*)(d_in + a_core), (const unsigned char*)(d_in + a_skip), (const unsigned char*)(d_in + a_oc),
                               (const unsigned char*)(d_in + a_oh), (const unsigned char*)(d_in + a_og), (const unsigned char*)(d_in + a_oo), d_keys);
        }
        SP_HIP_CHECK(ctx, hipGetLastError());
        SP_HIP_CHECK(ctx, hipMemcpyAsync(h_keys, d_keys, total * 8, hipMemcpyDeviceToHost, ctx->stream));
        SP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        keys.assign(h_keys, h_keys + total);
    }
    std::vector<unsigned long long> none;
    size_t at = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (rcs[i] != SP_OK) continue;
        const K6Prep& q = prep[i];
        if (q.H <= 0) { none.assign((size_t)q.n_cells, K6_NOKEY); k6_combine(problems[i], q, none.data(), &results[i]); continue; }
        k6_combine(problems[i], q, keys.data() + desc[at].cell_base, &results[i]);
        ++at;
    }
    if (problem_rc) for (uint32_t i = 0; i < n; ++i) problem_rc[i] = rcs[i];
    if (rc != SP_OK) ctx->err = first_err;
    return rc;
}

extern "C" int32_t sp_variant_solve(sp_ctx* ctx, const sp_variant_problem* p, sp_variant_result* res) {
    if (!ctx || !p || !res) return SP_ERR_INVALID_ARG;
    return sp_variant_solve_batch(ctx, 1, &p, res, nullptr);
}

// ---------------------------------------------------------------- the N best candidates (the definition: include/starphase_hip.h)
// All problems of the batch in one launch pair: the tables of the solve plus hap_is_core and the SV labels go up in one copy, k6_alt_kernel leaves N
// records per workgroup, k6_alt_select_kernel one list per problem, n * (N records + one info) come down in one copy.  Device memory: the tables and
// workgroups x N records, whatever n_comb is; every buffer is pooled (k6_alt_*), so a warm context allocates nothing and the solve's pools stay as they are.
extern "C" int32_t sp_variant_alternatives_batch(sp_ctx* ctx, uint32_t n, const sp_variant_problem* const* problems, uint32_t n_best, sp_variant_alt* alts,
                                                 sp_variant_alt_info* infos, int32_t* problem_rc) {
    if (!ctx) return SP_ERR_INVALID_ARG;
    if (n_best < 1 || n_best > K6_ALT_MAXN) return sp_fail(ctx, SP_ERR_INVALID_ARG, "sp_variant_alternatives: n_best must be 1 .. 64");
    if (n && (!problems || !alts || !infos)) return sp_fail(ctx, SP_ERR_INVALID_ARG, "sp_variant_alternatives_batch: null argument");
    for (uint32_t i = 0; i < n; ++i) if (!problems[i]) return sp_fail(ctx, SP_ERR_INVALID_ARG, "sp_variant_alternatives_batch: null problem");
    if (n == 0) return SP_OK;
    (void)hipSetDevice(ctx->device);
    const uint32_t N = n_best;
    std::vector<int32_t> rcs(n, SP_OK);
    std::string first_err; int32_t rc = SP_OK;
    std::vector<K6AltDesc> desc; std::vector<uint32_t> which;
    std::vector<uint8_t> ms, need, core, skip, hc, oc, oh, og, oo, osv, osd;
    std::memset(alts, 0, sizeof(sp_variant_alt) * (size_t)n * N);
    std::memset(infos, 0, sizeof(sp_variant_alt_info) * (size_t)n);
    {
        K6Prep q;
        for (uint32_t i = 0; i < n; ++i) {
            rcs[i] = k6_prep(ctx, problems[i], q);
            if (rcs[i] != SP_OK) { if (rc == SP_OK) { rc = rcs[i]; first_err = ctx->err; } continue; }
            const sp_variant_problem* p = problems[i];
            const int H1 = std::max(1, q.H), O1 = std::max(1, q.NO);
            std::vector<uint8_t> hap_core((size_t)H1, 1), svd((size_t)O1, 0xFF); std::vector<int32_t> sv((size_t)O1, -1);
            for (int h = 0; h < q.H; ++h) hap_core[h] = p->hap_is_core[h] ? 1 : 0;
            std::vector<int32_t> seen;                                  // the labels of the problem in first-seen order: at most one per observation
            for (int o = 0; o < q.NO; ++o) {
                const int32_t l = p->obs_sv_label[o];
                if (l < 0) continue;
                size_t k = 0; while (k < seen.size() && seen[k] != l) ++k;
                if (k == seen.size()) seen.push_back(l);
                sv[o] = l; svd[o] = (uint8_t)k;
            }
            K6AltDesc d; std::memset(&d, 0, sizeof d);
            d.n_haps = q.H; d.n_obs = q.NO; d.n_sides = q.n_sides; d.n_comb = q.n_comb;
            d.off_ms = (uint32_t)ms.size(); d.off_h = (uint32_t)skip.size(); d.off_o = (uint32_t)oc.size();
            append(ms, q.match_slot); append(need, q.slot_need); append(core, q.slot_core); append(skip, q.hap_skip); append(hc, hap_core);
            append(oc, q.obs_core); append(oh, q.obs_het); append(og, q.obs_group); append(oo, q.obs_orient); append(osv, sv); append(osd, svd);
            desc.push_back(d); which.push_back(i);
        }
    }
    if (!desc.empty()) {
        // the grid: eight one-wave workgroups per CU, shared out evenly; a problem never gets more workgroups than it has assignments
        const uint32_t P = (uint32_t)desc.size();
        const uint64_t share = std::max<uint64_t>(1, (uint64_t)std::max(1, ctx->num_cus) * 8 / P);
        uint32_t total_wg = 0;
        for (K6AltDesc& d : desc) { d.wg_base = total_wg; d.wg_count = (uint32_t)std::min<uint64_t>(d.n_comb, share); total_wg += d.wg_count; }
        size_t bytes = 0;
        auto place = [&](size_t b) { const size_t at = (bytes + 15) & ~(size_t)15; bytes = at + b; return at; };
        const size_t a_desc = place(desc.size() * sizeof(K6AltDesc)), a_ms = place(ms.size()), a_need = place(need.size()), a_core = place(core.size()), a_skip = place(skip.size());
        const size_t a_hc = place(hc.size()), a_oc = place(oc.size()), a_oh = place(oh.size()), a_og = place(og.size()), a_oo = place(oo.size()), a_osv = place(osv.size()), a_osd = place(osd.size());
        const size_t rec_bytes = (size_t)total_wg * N * sizeof(K6Cand), part_bytes = rec_bytes + (size_t)total_wg * sizeof(K6Part);
        const size_t alt_bytes = (size_t)P * N * sizeof(sp_variant_alt), out_bytes = alt_bytes + (size_t)P * sizeof(sp_variant_alt_info);
        uint8_t* h_in = (uint8_t*)sp_host_pool(ctx, "k6_alt_in", bytes + 16); uint8_t* d_in = (uint8_t*)sp_pool(ctx, "k6_alt_in", bytes + 16);
        uint8_t* d_part = (uint8_t*)sp_pool(ctx, "k6_alt_part", part_bytes);
        uint8_t* d_out = (uint8_t*)sp_pool(ctx, "k6_alt_out", out_bytes); uint8_t* h_out = (uint8_t*)sp_host_pool(ctx, "k6_alt_out", out_bytes);
        if (!h_in || !d_in || !d_part || !d_out || !h_out) return sp_fail(ctx, SP_ERR_OUT_OF_MEMORY, "variant alternatives buffers");
        auto put = [&](size_t at, const void* src, size_t b) { if (b) std::memcpy(h_in + at, src, b); };
        put(a_desc, desc.data(), desc.size() * sizeof(K6AltDesc)); put(a_ms, ms.data(), ms.size()); put(a_need, need.data(), need.size()); put(a_core, core.data(), core.size());
        put(a_skip, skip.data(), skip.size()); put(a_hc, hc.data(), hc.size()); put(a_oc, oc.data(), oc.size()); put(a_oh, oh.data(), oh.size()); put(a_og, og.data(), og.size());
        put(a_oo, oo.data(), oo.size()); put(a_osv, osv.data(), osv.size()); put(a_osd, osd.data(), osd.size());
        SP_HIP_CHECK(ctx, hipMemcpyAsync(d_in, h_in, bytes, hipMemcpyHostToDevice, ctx->stream));
        const K6AltDesc* d_desc = (const K6AltDesc*)(d_in + a_desc);
        K6Cand* d_rec = (K6Cand*)d_part; K6Part* d_pp = (K6Part*)(d_part + rec_bytes);
        {
            ProfScope ps(ctx, "k6_alt", total_wg);
            hipLaunchKernelGGL(k6_alt_kernel, dim3(total_wg), dim3(64), 0, ctx->stream, P, (int)N, d_desc, (const signed char*)(d_in + a_ms),
                               (const unsigned long long*)(d_in + a_need), (const unsigned long long*)(d_in + a_core), (const unsigned char*)(d_in + a_skip),
                               (const unsigned char*)(d_in + a_hc), (const unsigned char*)(d_in + a_oc), (const unsigned char*)(d_in + a_oh), (const unsigned char*)(d_in + a_og),
                               (const unsigned char*)(d_in + a_oo), (const int*)(d_in + a_osv), (const unsigned char*)(d_in + a_osd), d_rec, d_pp);
        }
        SP_HIP_CHECK(ctx, hipGetLastError());
        {
            ProfScope ps(ctx, "k6_alt_select", P);
            hipLaunchKernelGGL(k6_alt_select_kernel, dim3(P), dim3(64), 0, ctx->stream, (int)N, d_desc, (const K6Cand*)d_rec, (const K6Part*)d_pp,
                               (sp_variant_alt*)d_out, (sp_variant_alt_info*)(d_out + alt_bytes));
        }
        SP_HIP_CHECK(ctx, hipGetLastError());
        SP_HIP_CHECK(ctx, hipMemcpyAsync(h_out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
        SP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        for (uint32_t k = 0; k < P; ++k) {
            std::memcpy(alts + (size_t)which[k] * N, h_out + (size_t)k * N * sizeof(sp_variant_alt), (size_t)N * sizeof(sp_variant_alt));
            std::memcpy(infos + which[k], h_out + alt_bytes + (size_t)k * sizeof(sp_variant_alt_info), sizeof(sp_variant_alt_info));
        }
    }
    if (problem_rc) for (uint32_t i = 0; i < n; ++i) problem_rc[i] = rcs[i];
    if (rc != SP_OK) ctx->err = first_err;
    return rc;
}

extern "C" int32_t sp_variant_alternatives(sp_ctx* ctx, const sp_variant_problem* p, uint32_t n_best, sp_variant_alt* alts, sp_variant_alt_info* info) {
    if (!ctx || !p || !alts || !info) return SP_ERR_INVALID_ARG;
    return sp_variant_alternatives_batch(ctx, 1, &p, n_best, alts, info, nullptr);
}

// het_split of solve_diplotype (src/diplotyper.rs:1263-1317): the two observed haplotypes of het assignment `comb` as problem variant ids --
// the homozygous variants first, then the heterozygous ones in call order
void spi_het_split(const sp_variant_problem& p, int32_t comb, std::vector<int32_t>& h1, std::vector<int32_t>& h2) {
    h1.clear();
    for (int o = 0; o < p.n_obs; ++o) if (p.obs_gt[o] == SP_GT_HOM_ALT) h1.push_back(p.obs_var[o]);
    h2 = h1;
    int combo_index = 0;
    std::map<int64_t, int> lookup;
    for (int o = 0; o < p.n_obs; ++o) {
        if (p.obs_gt[o] == SP_GT_HOM_ALT) continue;
        int is_h1;
        const int64_t ps = p.obs_ps[o];
        if (ps >= 0) {
            auto it = lookup.find(ps);
            if (it == lookup.end()) { it = lookup.emplace(ps, (comb >> combo_index) & 1).first; ++combo_index; }
            is_h1 = it->second;
        } else { is_h1 = (comb >> combo_index) & 1; ++combo_index; }
        ((is_h1 != 0) == (p.obs_gt[o] != SP_GT_HET_FLIP) ? h1 : h2).push_back(p.obs_var[o]);
    }
}

// NormalizedPgxHaplotype::quant_match (src/data_types/normalized_variant.rs:431-479) on ids: matching / missing / extra variants
void spi_quant_match(const sp_variant_problem& p, int h, const std::vector<int32_t>& obs, std::vector<int32_t>& match, std::vector<int32_t>& missing,
                     std::vector<int32_t>& extra) {
    const int s0 = p.slot_off[h], s1 = p.slot_off[h + 1];
    std::vector<uint8_t> matched((size_t)(s1 - s0) + 1, 0);
    match.clear(); missing.clear(); extra.clear();
    for (int32_t v : obs) {
        int mi = -1;
        for (int s = s0; s < s1 && mi < 0; ++s)
            for (int x = p.alt_off[s]; x < p.alt_off[s + 1]; ++x) if (p.alt_var[x] == v) { mi = s - s0; break; }
        if (mi >= 0 && !matched[mi]) { matched[mi] = 1; match.push_back(v); } else extra.push_back(v);
    }
    for (int s = s0; s < s1; ++s) {
        bool has_none = false; int first_some = -1;
        for (int x = p.alt_off[s]; x < p.alt_off[s + 1]; ++x) { if (p.alt_var[x] < 0) has_none = true; else if (first_some < 0) first_some = p.alt_var[x]; }
        if (!(matched[s - s0] || has_none)) missing.push_back(first_some);
    }
}

namespace {
// the variants of side `side` of assignment `comb` under explanation `dip`, as (id, relationship): the matching, the missing, then the unexpected ones
int32_t k6_relations(const sp_variant_problem* p, int32_t comb, int32_t side, int32_t dip, std::vector<std::pair<int32_t, int32_t>>& out) {
    out.clear();
    if (!p || comb < 0 || side < 0 || side > 1 || dip >= p->n_haps || dip == -1 || p->n_obs < 0 || p->n_obs > K6_MAX_OBS) return SP_ERR_INVALID_ARG;
    {                                                        // comb < n_comb: one bit per phase set and per unphased het, the last one fixed (k6_prep)
        std::set<int64_t> sets; int groups = 0;
        for (int o = 0; o < p->n_obs; ++o) {
            if (p->obs_gt[o] == SP_GT_HOM_ALT) continue;
            if (p->obs_ps[o] < 0 || sets.insert(p->obs_ps[o]).second) ++groups;
        }
        if (groups > 24 || (unsigned long long)comb >= (groups ? 1ull << (groups - 1) : 1ull)) return SP_ERR_INVALID_ARG;
    }
    std::vector<int32_t> sides[2];
    spi_het_split(*p, comb, sides[0], sides[1]);
    const std::vector<int32_t>& mem = sides[side];
    if (dip >= 0) {
        std::vector<int32_t> m, mi, ex;
        spi_quant_match(*p, dip, mem, m, mi, ex);
        for (int32_t v : m) out.emplace_back(v, SP_REL_MATCH);
        for (int32_t v : mi) out.emplace_back(v, SP_REL_MISSING);
        for (int32_t v : ex) out.emplace_back(v, SP_REL_UNEXPECTED);
        return SP_OK;
    }
    // an SV label (:1414-1431): the first labelled member carries it, the first member of every distinct label behind it is unexpected
    std::vector<int32_t> rest; bool first = true;
    for (int32_t v : mem) {
        int32_t l = -1;
        for (int o = 0; o < p->n_obs; ++o) if (p->obs_var[o] == v) l = p->obs_sv_label[o];
        if (l < 0) continue;
        if (first) { if (-(l + 2) != dip) return SP_ERR_INVALID_ARG; out.emplace_back(v, SP_REL_MATCH); first = false; continue; }
        if (std::find(rest.begin(), rest.end(), l) != rest.end()) continue;
        rest.push_back(l); out.emplace_back(v, SP_REL_UNEXPECTED);
    }
    return first ? SP_ERR_INVALID_ARG : SP_OK;
}
} // namespace

extern "C" int32_t sp_variant_alt_relations(const sp_variant_problem* p, int32_t comb, int32_t side, int32_t dip, int32_t* ids, int32_t* rel, uint32_t cap, uint32_t* n) {
    std::vector<std::pair<int32_t, int32_t>> r;
    if (n) *n = 0;
    const int32_t rc = k6_relations(p, comb, side, dip, r);
    if (rc != SP_OK) return rc;
    if (n) *n = (uint32_t)r.size();
    if (r.size() > cap || (!r.empty() && (!ids || !rel))) return SP_ERR_CAPACITY;
    for (size_t k = 0; k < r.size(); ++k) { ids[k] = r[k].first; rel[k] = r[k].second; }
    return SP_OK;
}

// one gene's entry of variant_alternatives.json
extern "C" int32_t sp_variant_alternatives_json(const sp_variant_problem* p, const sp_variant_alt_info* info, const sp_variant_alt* alts, const char* const* hap_names,
                                                const char* const* hap_core_names, const char* const* sv_labels, uint32_t n_sv_labels, const char* const* var_names,
                                                char* out, uint64_t cap, uint64_t* needed) {
    if (!p || !info || (info->n_alts && !alts) || (p->n_haps > 0 && (!hap_names || !hap_core_names)) || (p->n_vars > 0 && !var_names)) return SP_ERR_INVALID_ARG;
    static const char* const FIELD[4] = {"core_missing", "core_unexpected", "sub_missing", "sub_unexpected"};
    auto score = [&](auto get) {
        spj::Value s = spj::object();
        for (int k = 0; k < 4; ++k) { const int64_t v = get(k); s.obj.emplace_back(FIELD[k], v == INT64_MAX ? spj::Value() : spj::num(v)); }
        return s;
    };
    spj::Value root = spj::object();
    root.obj.emplace_back("n_combinations", spj::unum(info->n_comb));
    root.obj.emplace_back("n_candidates", spj::unum(info->n_candidates));
    root.obj.emplace_back("best_score", score([&](int k) { return info->best_score[k]; }));
    spj::Value list = spj::array();
    for (uint32_t r = 0; r < info->n_alts; ++r) {
        const sp_variant_alt& a = alts[r];
        std::string name[2], core_name[2];
        for (int k = 0; k < 2; ++k) {
            const int32_t x = a.dip[k];
            if (x >= p->n_haps || (x < 0 && (x == -1 || (uint32_t)(-x - 2) >= n_sv_labels || !sv_labels))) return SP_ERR_INVALID_ARG;
            if (x >= 0) { name[k] = hap_names[x] ? hap_names[x] : ""; core_name[k] = hap_core_names[x] ? hap_core_names[x] : name[k]; }
            else { name[k] = sv_labels[-x - 2] ? sv_labels[-x - 2] : ""; core_name[k] = name[k].substr(0, name[k].find('.')); }      // build_core_allele_lookup (:378-399)
        }
        const bool exact_sub = !a.score[0] && !a.score[1] && !a.score[2] && !a.score[3], exact_core = !a.score[0] && !a.score[1];
        spj::Value e = spj::object();
        e.obj.emplace_back("rank", spj::unum((uint64_t)r + 1));               // 1: the best candidate
        e.obj.emplace_back("diplotype", spj::str(exact_sub ? name[0] + "/" + name[1] : exact_core ? core_name[0] + "/" + core_name[1] : std::string("NO_MATCH/NO_MATCH")));
        e.obj.emplace_back("called", spj::boolean((a.flags & SP_VAR_ALT_CALLED) != 0));
        e.obj.emplace_back("shadowed", spj::boolean((a.flags & SP_VAR_ALT_SHADOWED) != 0));
        e.obj.emplace_back("score", score([&](int k) { return a.score[k]; }));
        e.obj.emplace_back("combination", spj::num(a.comb));
        for (int k = 0; k < 2; ++k) {
            std::vector<std::pair<int32_t, int32_t>> rel;
            const int32_t rc = k6_relations(p, a.comb, k, a.dip[k], rel);
            if (rc != SP_OK) return rc;
            spj::Value hap = spj::object(), missing = spj::array(), unexpected = spj::array();
            for (auto& vr : rel) {
                if (vr.first < 0 || vr.first >= p->n_vars) return SP_ERR_INVALID_ARG;
                std::string nm = var_names[vr.first] ? var_names[vr.first] : "";
                if (a.dip[k] < 0) for (int o = 0; o < p->n_obs; ++o) if (p->obs_var[o] == vr.first && p->obs_sv_label[o] >= 0 && (uint32_t)p->obs_sv_label[o] < n_sv_labels) nm = sv_labels[p->obs_sv_label[o]];
                if (vr.second == SP_REL_MISSING) missing.arr.push_back(spj::str(nm)); else if (vr.second == SP_REL_UNEXPECTED) unexpected.arr.push_back(spj::str(nm));
            }
            hap.obj.emplace_back("haplotype", spj::str(name[k]));
            hap.obj.emplace_back("score", score([&](int f) { return (int64_t)a.side_score[k][f]; }));
            hap.obj.emplace_back("missing", std::move(missing)); hap.obj.emplace_back("unexpected", std::move(unexpected));
            e.obj.emplace_back(k ? "hap2" : "hap1", std::move(hap));
        }
        list.arr.push_back(std::move(e));
    }
    root.obj.emplace_back("alternatives", std::move(list));
    std::string text;
    spj::write_pretty(text, root);
    if (needed) *needed = text.size() + 1;
    if (out && cap) { const size_t k = std::min<size_t>(text.size(), (size_t)cap - 1); std::memcpy(out, text.data(), k); out[k] = 0; if (k < text.size()) return SP_ERR_CAPACITY; }
    return SP_OK;
}

"""Every chain pair of a find_best_chain_pair problem scored in plain Python, for sp_cyp_best_chain_pairs (the N best pairs under (score, i, j)).

Written from the contract of include/starphase_hip.h and src/cyp2d6/chaining.rs:409-534 (the scoring loop), :683-731 (containment_score) and :854-903
(get_multinomial_score) with multinomial_ln_pmf (src/util/stats.rs:11-37).  The problems it judges have ignore_chain_label_limits = 1 and infer_connections = 0,
so it needs no label grammar: every allowed region (not UNKNOWN, not FalseAllele) counts for the lasso term, every region normalises, and the unexpected-chain and
inferred-edge penalties are 0 by definition.  The chains come from the caller (the library's sp_cyp_possible_chains).

f64 sums are made in the reference's operand order.  ln n! is what the library's host table holds: log of the running product up to 170!, lgamma beyond -- libm's
lgamma, the function the library calls (math.lgamma is CPython's own code and may differ in the last bit); ln(c / total) is math.log of the quotient."""
import ctypes
import ctypes.util
import math

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.lgamma.restype = ctypes.c_double
_libm.lgamma.argtypes = [ctypes.c_double]

UNKNOWN, DELETION, FALSE_ALLELE = 0, 7, 9


def ln_factorials(n):
    out, f = [], 1.0
    for k in range(n):
        if 2 <= k <= 170:
            f *= float(k)
        out.append(math.log(f) if k <= 170 else _libm.lgamma(float(k) + 1.0))
    return out


def round_half_away(x):
    """f64::round for x >= 0"""
    r = math.floor(x)
    return int(r) + 1 if x - r >= 0.5 else int(r)


def is_sub(hay, needle):
    n = len(needle)
    return any(hay[s:s + n] == needle for s in range(len(hay) - n + 1))


def score_pairs(inp, chains):
    """inp: the flattened problem (oracle_ffi.ChainInputs); chains: lists of region indices in enumeration order.
    Returns the valid pairs i <= j sorted by (score, i, j): dicts with index1, index2, score, ln_ed_penalty, mn_llh_penalty, allele_expected_penalty,
    unexpected_chain_penalty, inferred_chain_penalty, edit_distance, unmet_observations, hap_counts, hap_weights, partial_cost."""
    assert inp.ignore == 1 and inp.infer == 0
    H = inp.H
    types = [int(t) for t in inp.types]
    lasso, ln_ed, _unexpected, _inferred = inp.penalties
    n_reads = max(len(inp.chain_names), len(inp.score_names))
    rwo = [int(v) for v in inp.read_w_off] if len(inp.read_w_off) == n_reads + 1 else [0] * (n_reads + 1)
    rco = [int(v) for v in inp.read_chain_off] if len(inp.read_chain_off) == n_reads + 1 else [0] * (n_reads + 1)
    co, items = [int(v) for v in inp.chain_off], [int(v) for v in inp.chain_items]
    reads = []                                            # per read: rows of (ed, ov) per region, optimum, worst
    for r in range(n_reads):
        ed = [[int(v) for v in inp.w_ed[row]] for row in range(rwo[r], rwo[r + 1])]
        ov = [[float(v) for v in inp.w_ov[row]] for row in range(rwo[r], rwo[r + 1])]
        reads.append((ed, ov, sum(min(row) for row in ed), sum(max(row) for row in ed)))
    observed = [[items[co[c]:co[c + 1]] for c in range(rco[r], rco[r + 1])] for r in range(n_reads)]
    bound = sum(max(row) for _, ov, _, _ in reads for row in ov)
    lf = ln_factorials(int(math.ceil(bound)) + H + 2)
    chains = [list(c) for c in chains]
    # per (read, chain): the window totals (they do not depend on the partner chain)
    totals = [[[sum(ed[x][ch[s + x]] for x in range(len(ed))) for s in range(len(ch) - len(ed) + 1)] for ch in chains] for ed, _, _, _ in reads]
    out = []
    for i in range(len(chains)):
        for j in range(i, len(chains)):
            counts = [0] * H
            for h in chains[i] + chains[j]:
                counts[h] += 1
            unexpected_alleles = sum(counts[h] - 1 for h in range(H) if types[h] not in (UNKNOWN, FALSE_ALLELE) and counts[h] > 0)
            allele_expected_penalty = lasso * float(unexpected_alleles)
            unmet = sum(1 for obs in observed if not any(is_sub(chains[i], ch) or is_sub(chains[j], ch) for ch in obs))
            combined, weights = 0, [0.0] * H
            for r, (ed, ov, optimum, worst) in enumerate(reads):
                best, best_chains = 2 * worst, []
                for which in (i, j):
                    for s, total in enumerate(totals[r][which]):
                        if total < best:
                            best, best_chains = total, []
                        if total == best:
                            best_chains.append(chains[which][s:s + len(ed)])
                combined += best - optimum
                if best_chains:
                    split = 1.0 / float(len(best_chains))
                    for ch in best_chains:
                        for x, con in enumerate(ch):
                            weights[con] += split * ov[x][con]
            ln_ed_penalty = float(combined) * ln_ed
            reduced = [h for h in range(H) if counts[h] > 0]                 # every region normalises when the label limits are ignored
            coverage = [round_half_away(weights[h]) for h in reduced]
            if not reduced or sum(coverage) == 0:
                both_deleted = any(types[h] == DELETION for h in chains[i]) and any(types[h] == DELETION for h in chains[j])
                if inp.normalize_all or not both_deleted:
                    continue
                mn = 0.0
            else:
                total_count = sum(counts[h] for h in reduced)
                coeff = lf[sum(coverage)]
                for c in coverage:
                    coeff -= lf[c]
                acc = 0.0
                for h, c in zip(reduced, coverage):
                    acc = acc + float(c) * math.log(float(counts[h]) / float(total_count))
                mn = abs(coeff + acc)
            score = ln_ed_penalty + mn + allele_expected_penalty + 0.0 + 0.0
            out.append({"index1": i, "index2": j, "score": score, "ln_ed_penalty": ln_ed_penalty, "mn_llh_penalty": mn,
                        "allele_expected_penalty": allele_expected_penalty, "unexpected_chain_penalty": 0.0, "inferred_chain_penalty": 0.0,
                        "edit_distance": combined, "unmet_observations": unmet, "hap_counts": counts, "hap_weights": weights,
                        "partial_cost": allele_expected_penalty + 0.0 + 0.0})
    out.sort(key=lambda e: (e["score"], e["index1"], e["index2"]))
    return out

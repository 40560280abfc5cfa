"""A chain pair read by read, and the observed-chain table, in plain Python: the reference of sp_cyp_chain_pair_reads and sp_cyp_observed_chains.

Written from the contract in include/starphase_hip.h and from src/cyp2d6/chaining.rs:683-731 (containment_score), :427-440 (the is_sub loop), src/cyp2d6/caller.rs:544-550
(chain_frequency) and src/cyp2d6/visualization.rs:32-45 (the node and edge totals).  It imports nothing from the library; the chains come from the caller (the
library's sp_cyp_possible_chains)."""
from chain_pairs_ref import is_sub

U64 = (1 << 64) - 1


def flat(inp):
    """the reads of an oracle_ffi.ChainInputs: per read (ed rows, ov rows, observed chains)"""
    n_reads = max(len(inp.chain_names), len(inp.score_names))
    rwo = [int(v) for v in inp.read_w_off] if len(inp.read_w_off) == n_reads + 1 else [0] * (n_reads + 1)
    rco = [int(v) for v in inp.read_chain_off] if len(inp.read_chain_off) == n_reads + 1 else [0] * (n_reads + 1)
    co, items = [int(v) for v in inp.chain_off], [int(v) for v in inp.chain_items]
    out = []
    for r in range(n_reads):
        ed = [[int(v) for v in inp.w_ed[row]] for row in range(rwo[r], rwo[r + 1])]
        ov = [[float(v) for v in inp.w_ov[row]] for row in range(rwo[r], rwo[r + 1])]
        out.append((ed, ov, [items[co[c]:co[c + 1]] for c in range(rco[r], rco[r + 1])]))
    return out


def pair_read(chain_i, chain_j, ed, observed):
    """one record: dict(mask1, mask2, excess_ed, n_best, supported)"""
    wl = len(ed)
    optimum = sum(min(row) for row in ed)
    worst = sum(max(row) for row in ed)
    best, masks = 2 * worst, [0, 0]
    for which, chain in enumerate((chain_i, chain_j)):
        if len(chain) < wl:
            continue
        for s in range(len(chain) - wl + 1):
            total = sum(ed[x][chain[s + x]] for x in range(wl))
            if total < best:
                best, masks = total, [0, 0]
            if total == best:
                masks[which] |= (1 << s) & U64
    supported = any(is_sub(chain_i, ch) or is_sub(chain_j, ch) for ch in observed)
    return {"mask1": masks[0], "mask2": masks[1], "excess_ed": best - optimum, "n_best": bin(masks[0]).count("1") + bin(masks[1]).count("1"),
            "supported": 1 if supported else 0}


def pair_reads(inp, chains, pairs):
    """[n_pairs][n_reads] records"""
    reads = flat(inp)
    return [[pair_read(list(chains[i]), list(chains[j]), ed, obs) for ed, _, obs in reads] for i, j in pairs]


def hap_weights(inp, chains, pair, records):
    """the coverage sums of a pair from its records: the reads in order, chain index1's starts ascending, then index2's, rows ascending; split * ov[x][con]"""
    weights = [0.0] * inp.H
    for (ed, ov, _), rec in zip(flat(inp), records):
        if not int(rec["n_best"]):
            continue
        split = 1.0 / float(int(rec["n_best"]))
        for which, mask in ((pair[0], int(rec["mask1"])), (pair[1], int(rec["mask2"]))):
            for s in range(64):
                if mask >> s & 1:
                    for x in range(len(ed)):
                        con = chains[which][s + x]
                        weights[con] += split * ov[x][con]
    return weights


def observed_table(inp):
    """(chains in lexicographic order, their frequencies, single_counts [H], edges in lexicographic order, their weights)"""
    freq = {}
    for _, _, observed in flat(inp):                       # the reads in problem order
        if not observed:
            continue
        weight = 1.0 / float(len(observed))
        for ch in observed:
            freq[tuple(ch)] = freq.get(tuple(ch), 0.0) + weight
    chains = sorted(freq)
    single = [0.0] * inp.H
    edges = {}
    for ch in chains:                                      # BTreeMap order
        for h in ch:
            single[h] += freq[ch]
        for a, b in zip(ch, ch[1:]):
            edges[(a, b)] = edges.get((a, b), 0.0) + freq[ch]
    order = sorted(edges)
    return [list(c) for c in chains], [freq[c] for c in chains], single, order, [edges[e] for e in order]

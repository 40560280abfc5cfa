"""The haplotype list of sp_pileup_hap_batch / sp_align_pileup_hap_batch, stated in plain Python: op rows as sp_affine_align_batch returns them and the query strings
-> the column table, the contested columns, every aligned pair's calls there, the records and the heads.  The definition of include/starphase_hip.h applied literally;
nothing of the library is used."""
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
HAP_COLS = 64
FIELDS = ("target", "n_cols", "count", "first_pair", "w")
HEAD_FIELDS = ("first_record", "n_records", "n_cols", "n_cols_total")


def walk(pairs, aln, cigar, n_cigar, queries, need_score=False):
    """per aligned pair (n_cigar > 0; with need_score also score > 0): (pair index, target, {column: low code}, {columns with an 'I' run behind them})"""
    out = []
    for p, pr in enumerate(pairs):
        if int(n_cigar[p]) == 0 or (need_score and int(aln[p]["score"]) <= 0):
            continue
        q, t = queries[pr[0]], pr[1]
        j, i = int(aln[p]["b_start"]), int(aln[p]["a_start"])
        low, ins = {}, set()
        for k in range(int(n_cigar[p])):
            op, n = int(cigar[p][k]) & 15, int(cigar[p][k]) >> 4
            if op == 1:
                if j - 1 >= 0:
                    ins.add(j - 1)
                i += n
            elif op == 2:
                for c in range(j, j + n):
                    low[c] = 6
                j += n
            else:
                for x in range(n):
                    low[j + x] = 1 if op == 7 else 2 + CODE.get(q[i + x], 0)
                j += n
                i += n
        out.append((p, t, low, ins))
    return out


def table(walked, lengths):
    """per target: per column [depth, eq, x0, x1, x2, x3, del, ins]"""
    tab = [[[0] * 8 for _ in range(int(n))] for n in lengths]
    for p, t, low, ins in walked:
        for c, v in low.items():
            col = tab[t][c]
            col[0] += 1
            col[1 if v == 1 else 6 if v == 6 else v] += 1
        for c in ins:
            if c < len(tab[t]):
                tab[t][c][7] += 1
    return tab


def contested(cols):
    return [j for j, c in enumerate(cols) if (c[0] > 0 and 2 * c[1] <= c[0]) or 2 * c[7] > c[0]]


def records(pairs, aln, cigar, n_cigar, queries, lengths, need_score=False):
    """-> (records as tuples in FIELDS order with w a 4-tuple, heads as tuples in HEAD_FIELDS order, the table)"""
    walked = walk(pairs, aln, cigar, n_cigar, queries, need_score)
    tab = table(walked, lengths)
    recs, heads = [], []
    for t in range(len(lengths)):
        all_cols = contested(tab[t])
        used = all_cols[:HAP_COLS]
        pats = {}
        if used:
            for p, tt, low, ins in walked:
                if tt != t:
                    continue
                v = 0
                for k, c in enumerate(used):
                    v |= (low.get(c, 0) | (8 if c in ins else 0)) << (4 * k)
                e = pats.setdefault(v, [0, p])
                e[0] += 1
                e[1] = min(e[1], p)
        mine = sorted(((t, len(used), e[0], e[1], v) for v, e in pats.items()), key=lambda r: (-r[2], r[4]))
        heads.append((len(recs), len(mine), len(used), len(all_cols)))
        recs += [r[:4] + (tuple((r[4] >> (64 * i)) & ((1 << 64) - 1) for i in range(4)),) for r in mine]
    return recs, heads, tab


def as_rows(arr):
    """a HAP_DTYPE array as the same tuples"""
    return [(int(r["target"]), int(r["n_cols"]), int(r["count"]), int(r["first_pair"]), tuple(int(x) for x in r["w"])) for r in arr]


def as_heads(arr):
    return [tuple(int(r[f]) for f in HEAD_FIELDS) for r in arr]


def call(rec, k):
    """call k of a record tuple"""
    return (rec[4][k // 16] >> (4 * (k % 16))) & 15


def text(rec):
    """the calls as sp_support_hap_string writes them"""
    return "".join("?=ACGT-?"[call(rec, k) & 7] + ("+" if call(rec, k) & 8 else "") for k in range(rec[1]))


def check_invariants(recs, heads, cols, n_aligned=None):
    """the three invariants of the header against a column table of the library (cols: one PILEUP_DTYPE array per target)"""
    for t, (first, n, K, total) in enumerate(heads):
        mine = recs[first:first + n]
        used = [j for j, c in enumerate(cols[t]) if (int(c["depth"]) > 0 and 2 * int(c["eq"]) <= int(c["depth"])) or 2 * int(c["ins"]) > int(c["depth"])]
        assert total == len(used) and K == min(total, HAP_COLS)
        assert all(r[0] == t and r[1] == K for r in mine)
        if K > 0 and n_aligned is not None:
            assert sum(r[2] for r in mine) == n_aligned[t]
        for k, j in enumerate(used[:K]):
            c = cols[t][j]
            got = [0] * 8
            ins = 0
            for r in mine:
                got[call(r, k) & 7] += r[2]
                ins += r[2] if call(r, k) & 8 else 0
            assert got[1] == int(c["eq"]) and got[2:6] == [int(x) for x in c["x"]] and got[6] == int(c["del"]) and got[7] == 0 and ins == int(c["ins"])
            assert sum(got[1:7]) == int(c["depth"])

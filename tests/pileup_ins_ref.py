"""The insertion list of sp_pileup_ins_batch / sp_align_pileup_ins_batch, stated in plain Python: op rows as sp_affine_align_batch returns them and the query
strings -> the records.  A dict keyed by (column, the inserted string itself) up to 64 bases and by (column, the stated key) beyond; the FNV-1a is computed here."""
import numpy as np

CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
FNV_BASIS, FNV_PRIME, MASK = 0xCBF29CE484222325, 0x100000001B3, (1 << 64) - 1
FIELDS = ("col", "len", "count", "p0", "p1", "h", "first_pair", "first_qpos", "n_other", "reserved_")


def key_of(s):
    """(len, p0, p1, h) of an inserted string over ACGT"""
    p0 = p1 = 0
    h = FNV_BASIS
    for i, ch in enumerate(s):
        c = CODE[ch]
        if i < 32:
            p0 |= c << (2 * i)
        elif i < 64:
            p1 |= c << (2 * (i - 32))
        h = ((h ^ c) * FNV_PRIME) & MASK
    return len(s), p0, p1, h


def records(pairs, aln, cigar, n_cigar, queries, col_offset, need_score=False):
    """-> list of tuples in FIELDS order, in the list's order.  pairs = [(query, target, ...)]; a pair with n_cigar 0 (or, with need_score, score <= 0) is left out."""
    table, other = {}, {}
    for p, pr in enumerate(pairs):
        if int(n_cigar[p]) == 0 or (need_score and int(aln[p]["score"]) <= 0):
            continue
        q, t = queries[pr[0]], pr[1]
        j, i = int(aln[p]["b_start"]), int(aln[p]["a_start"])
        for k in range(int(n_cigar[p])):
            op, n = int(cigar[p][k]) & 15, int(cigar[p][k]) >> 4
            if op == 1:
                if j - 1 >= 0:
                    col, s = int(col_offset[t]) + j - 1, q[i:i + n]
                    if any(ch not in CODE for ch in s):
                        other[col] = other.get(col, 0) + 1
                    else:
                        ident = (col, s) if n <= 64 else (col,) + key_of(s)
                        e = table.setdefault(ident, [0, p, i, key_of(s)])
                        e[0] += 1
                        if p < e[1]:
                            e[1], e[2] = p, i
                i += n
            elif op == 2:
                j += n
            else:
                j += n
                i += n
    rows = [(ident[0], key[0], e, key[1], key[2], key[3], p, i) for ident, (e, p, i, key) in table.items()]
    rows.sort(key=lambda r: (r[0], -r[2], r[1], r[3], r[4], r[5]))
    out, seen = [], set()
    for r in rows:
        first = r[0] not in seen
        seen.add(r[0])
        out.append(r + (other.get(r[0], 0) if first else 0, 0))
    for col, k in other.items():
        if col not in seen:
            out.append((col, 0, 0, 0, 0, 0, 0, 0, k, 0))
    out.sort(key=lambda r: r[0])                                                # (stable: a column's records keep their order)
    return out


def as_rows(arr):
    """an INS_DTYPE array as the same tuples"""
    return [tuple(int(r[f]) for f in FIELDS) for r in arr]


def ins_per_column(rows):
    """column -> count + n_other summed over its records: what sp_pileup_col.ins holds"""
    out = {}
    for r in rows:
        out[r[0]] = out.get(r[0], 0) + r[2] + r[8]
    return out

"""The pileup of sp_pileup_batch and the rule of sp_support_summary restated in plain Python: one loop over the ops of every alignment and one dict of columns per
target.  It walks the op arrays and the ASCII queries; there are no run chunks and no tiles here, so it shares nothing with the kernel's schedule."""
import numpy as np

CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
FIELDS = ("depth", "eq", "x0", "x1", "x2", "x3", "del", "ins")


def pileup(queries, target_lens, pairs, aln, cigar, n_cigar):
    """queries: ASCII strings; target_lens: length per target; pairs: (a, b, ...) rows; aln: records with a_start / b_start; cigar[p][k] = len << 4 | op
    -> per target an int array [length][8] in the order of FIELDS"""
    cols = [dict() for _ in target_lens]

    def bump(t, j, field):
        cols[t].setdefault(j, [0] * 8)[field] += 1

    for p, pr in enumerate(pairs):
        a, t = int(pr[0]), int(pr[1])
        j, q = int(aln[p]["b_start"]), int(aln[p]["a_start"])
        for k in range(int(n_cigar[p])):
            op, n = int(cigar[p][k]) & 15, int(cigar[p][k]) >> 4
            if op == 1:                                  # insertion: one per op, on the column before it
                bump(t, j - 1, 7)
                q += n
                continue
            for _ in range(n):
                bump(t, j, 0)
                if op == 7:
                    bump(t, j, 1)
                    q += 1
                elif op == 8:
                    bump(t, j, 2 + CODE.get(queries[a][q], 0))   # a base outside ACGT is held with code 0
                    q += 1
                elif op == 2:
                    bump(t, j, 6)
                else:
                    raise ValueError(f"op {op}")
                j += 1
    out = []
    for t, length in enumerate(target_lens):
        tab = np.zeros((length, 8), np.int64)
        for j, v in cols[t].items():
            assert 0 <= j < length, (t, j, length)
            tab[j] = v
        out.append(tab)
    return out


def as_table(cols):
    """a PILEUP_DTYPE array of the binding as an int array [length][8] in the order of FIELDS"""
    tab = np.zeros((len(cols), 8), np.int64)
    tab[:, 0], tab[:, 1], tab[:, 2:6], tab[:, 6], tab[:, 7] = cols["depth"], cols["eq"], cols["x"], cols["del"], cols["ins"]
    return tab


def contested(tab):
    """columns whose consensus base, or the absence of an insertion behind it, lacks a strict majority of the spanning members"""
    return [j for j in range(len(tab)) if (tab[j][0] > 0 and 2 * tab[j][1] <= tab[j][0]) or 2 * tab[j][7] > tab[j][0]]


def summary(tab, n_members, n_aligned):
    depth = sorted(int(d) for d in tab[:, 0])
    return dict(n_members=n_members, n_aligned=n_aligned, n_unaligned=n_members - n_aligned, length=len(tab),
                min_depth=depth[0] if depth else 0, median_depth=depth[(len(depth) - 1) // 2] if depth else 0, n_contested=len(contested(tab)))

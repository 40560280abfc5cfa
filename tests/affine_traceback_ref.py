"""The Python statement of sp_affine_align_batch: osp_affine_local of oracle/affine.c restated with back pointers, and the checks a CIGAR of that
DP has to pass.  The forward pass is the oracle's, line for line; every cell additionally remembers where each of its states came from, and the path
is walked back from the oracle's end cell (the first best cell by anti-diagonal, then by row) through those decisions:
  H     the diagonal, then E1, F1, E2, F2, each replacing only when strictly greater
  E, F  the gap is continued only where that was strictly better than opening one (so an F tie goes to the nearest opening)
  stop  at the cell the path started in: the diagonal step out of a cell with h.s <= 0
Ops are (length, op) with BAM's numbers: 7 '=', 8 'X' (also every column with an ambiguous base), 1 'I' (query only), 2 'D' (target only).
Pure Python, 10 - 20 us per cell: for small pairs only."""
import numpy as np

NEG = -(1 << 28)
MAP_HIFI = dict(a=1, b=4, q=6, e=2, q2=26, e2=1, sc_ambi=1)
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
H_DIAG, H_E1, H_F1, H_E2, H_F2, H_START, H_NONE = range(7)


def encode(seq):
    return [CODE.get(c, 4) for c in seq]


def affine_traceback(target, query, k0, band, a=1, b=4, q=6, e=2, q2=26, e2=1, sc_ambi=1):
    """target, query: strings; k0 = q_pos - t_pos (the negative of the library's diag) -> ((score, nm, t_start, t_end, q_start, q_end), [(len, op)])"""
    T, Q = encode(target), encode(query)
    tlen, qlen = len(T), len(Q)
    zero = ((0, 0, 0, 0, 0, 0), [])
    if tlen <= 0 or qlen <= 0:
        return zero
    B = 256 if band == 256 else 64
    klo = k0 - B // 2
    none = (NEG, 0, 0, 0)                                    # (s, nm, si, sj)
    H, E1, E2 = [none] * (B + 2), [none] * (B + 2), [none] * (B + 2)
    best, bi, bj, bnm, bsi, bsj = 0, -1, -1, 0, 0, 0
    i_lo, i_hi = max(0, -(klo + B - 1)), min(tlen - 1, qlen - 1 - klo)
    back = {}                                                # (i, l) -> (source of H, E1 continued, E2 continued, F1 continued, F2 continued, column is X)
    for i in range(i_lo, i_hi + 1):
        Hn, E1n, E2n = [none] * (B + 2), [none] * (B + 2), [none] * (B + 2)
        F1 = F2 = left = none
        ct = T[i]
        for l in range(B):
            j = i + klo + l
            if j < 0 or j >= qlen:
                F1 = F2 = left = none
                continue
            e1 = e2_ = none
            e1c = e2c = False
            if l + 1 < B:
                hu, eu, eu2 = H[l + 1], E1[l + 1], E2[l + 1]
                if hu[0] > NEG or eu[0] > NEG:
                    eo = hu[0] - q if hu[0] > NEG else NEG
                    if eu[0] > eo:
                        e1, e1c = (eu[0] - e, eu[1] + 1, eu[2], eu[3]), True
                    else:
                        e1 = (eo - e, hu[1] + 1, hu[2], hu[3])
                if hu[0] > NEG or eu2[0] > NEG:
                    eo2 = hu[0] - q2 if hu[0] > NEG else NEG
                    if eu2[0] > eo2:
                        e2_, e2c = (eu2[0] - e2, eu2[1] + 1, eu2[2], eu2[3]), True
                    else:
                        e2_ = (eo2 - e2, hu[1] + 1, hu[2], hu[3])
            f1 = f2 = none
            f1c = f2c = False
            if left[0] > NEG or F1[0] > NEG:
                fo = left[0] - q if left[0] > NEG else NEG
                if F1[0] > fo:
                    f1, f1c = (F1[0] - e, F1[1] + 1, F1[2], F1[3]), True
                else:
                    f1 = (fo - e, left[1] + 1, left[2], left[3])
            if left[0] > NEG or F2[0] > NEG:
                fo2 = left[0] - q2 if left[0] > NEG else NEG
                if F2[0] > fo2:
                    f2, f2c = (F2[0] - e2, F2[1] + 1, F2[2], F2[3]), True
                else:
                    f2 = (fo2 - e2, left[1] + 1, left[2], left[3])
            h = H[l]
            cq = Q[j]
            ambi = ct > 3 or cq > 3
            is_x = ambi or ct != cq
            sub = -sc_ambi if ambi else (a if ct == cq else -b)
            src = H_DIAG
            if h[0] <= 0:
                h, src = (0, 0, i, j), H_START
            h = (h[0] + sub, h[1] + (1 if is_x else 0), h[2], h[3])
            if e1[0] > h[0]:
                h, src = e1, H_E1
            if f1[0] > h[0]:
                h, src = f1, H_F1
            if e2_[0] > h[0]:
                h, src = e2_, H_E2
            if f2[0] > h[0]:
                h, src = f2, H_F2
            if h[0] <= 0:
                h, src = (0, 0, i, j), H_NONE
            Hn[l], E1n[l], E2n[l] = h, e1, e2_
            F1, F2, left = f1, f2, h
            back[(i, l)] = (src, e1c, e2c, f1c, f2c, is_x)
            if h[0] > best or (h[0] == best and h[0] > 0 and (i + j < bi + bj or (i + j == bi + bj and i < bi))):
                best, bi, bj, bnm, bsi, bsj = h[0], i, j, h[1], h[2], h[3]
        H, E1, E2 = Hn, E1n, E2n
    if best <= 0:
        return zero
    steps = []                                               # one op per column, last column first
    i, l, st = bi, bj - bi - klo, 0
    while True:
        src, e1c, e2c, f1c, f2c, is_x = back[(i, l)]
        if st == 0:
            if src in (H_DIAG, H_START):
                steps.append(8 if is_x else 7)
                if src == H_START:
                    assert (i, i + klo + l) == (bsi, bsj)
                    break
                i -= 1
                continue
            assert src != H_NONE
            st = src
        if st in (H_E1, H_E2):
            steps.append(2)
            cont = e1c if st == H_E1 else e2c
            i, l = i - 1, l + 1
        else:
            steps.append(1)
            cont = f1c if st == H_F1 else f2c
            l -= 1
        if not cont:
            st = 0
    steps.reverse()
    ops = []
    for op in steps:
        if ops and ops[-1][1] == op:
            ops[-1] = (ops[-1][0] + 1, op)
        else:
            ops.append((1, op))
    return (best, bnm, bsi, bi + 1, bsj, bj + 1), ops


def decode_ops(row, n):
    """a row of the library's cigar array -> [(len, op)]"""
    return [(int(w) >> 4, int(w) & 15) for w in row[:n]]


def check_ops(ops, target, query, t_start, t_end, q_start, q_end, a=1, b=4, q=6, e=2, q2=26, e2=1, sc_ambi=1):
    """What any CIGAR of the two-piece affine DP satisfies, checked without a second aligner: the ops consume exactly the two spans, every '=' column holds
    equal unambiguous bases and every 'X' column does not -> (X + I + D bases, two-piece affine score of the path)"""
    t = np.frombuffer(target.encode(), np.uint8)
    qq = np.frombuffer(query.encode(), np.uint8)
    acgt = np.zeros(256, bool)
    acgt[[65, 67, 71, 84]] = True
    i, j, nm, score = t_start, q_start, 0, 0
    prev = None
    for n, op in ops:
        assert n > 0 and op in (7, 8, 1, 2), (n, op)
        assert op != prev, "adjacent runs of one op"
        prev = op
        if op in (7, 8):
            assert i + n <= t_end and j + n <= q_end
            tt, qs = t[i:i + n], qq[j:j + n]
            clear = acgt[tt] & acgt[qs]
            same = clear & (tt == qs)
            if op == 7:
                assert same.all(), ("'=' over unequal or ambiguous bases", i, j, n)
                score += a * n
            else:
                assert not same.any(), ("'X' over equal bases", i, j, n)
                n_ambi = int((~clear).sum())
                score -= sc_ambi * n_ambi + b * (n - n_ambi)
                nm += n
            i += n; j += n
        else:
            score -= min(q + n * e, q2 + n * e2)
            nm += n
            if op == 2:
                i += n
            else:
                j += n
    assert (i, j) == (t_end, q_end), ("spans", (i, j), (t_end, q_end))
    return nm, score


def fuzz_pairs(rng, n):
    """small pairs that meet every rule of the traceback: substitutions, homopolymer indels, gaps of more than 20 bases (where the second piece 26 + l wins), N bases,
    pairs that do not align (unrelated sequences; a band beside the rectangle), and a diagonal a little (or far) off -> [(target, query, diag = t_pos - q_pos)]"""
    out = []
    for it in range(n):
        L = int(rng.integers(60, 401))
        base = list(rng.choice(list("ACGT"), L))
        kind = it % 8
        if kind in (1, 5):                                   # homopolymer runs to shrink and stretch
            for _ in range(int(rng.integers(1, 4))):
                p = int(rng.integers(5, L - 15)); base[p:p + 8] = base[p] * 8
        t = "".join(base)
        q = list(t)
        for _ in range(int(rng.integers(0, 7))):             # substitutions, some next to one another
            p = int(rng.integers(0, len(q))); q[p] = "ACGT"[("ACGT".index(q[p]) + int(rng.integers(1, 4))) % 4] if q[p] in "ACGT" else "A"
        if kind in (1, 5):
            for _ in range(int(rng.integers(1, 4))):
                p = int(rng.integers(1, len(q) - 1))
                if rng.random() < 0.5:
                    del q[p]
                else:
                    q.insert(p, q[p])
        if kind in (2, 6):                                   # a long gap on either side
            p, g = int(rng.integers(10, len(q) - 10)), int(rng.integers(21, 45))
            if rng.random() < 0.5:
                del q[p:p + g]
            else:
                q[p:p] = list(rng.choice(list("ACGT"), g))
        if kind == 3:                                        # ambiguous bases in either sequence
            for _ in range(int(rng.integers(1, 4))):
                p = int(rng.integers(0, len(q))); q[p] = "N"
            p = int(rng.integers(0, L)); t = t[:p] + "N" + t[p + 1:]
        q = "".join(q)
        if kind == 4:                                        # nothing in common
            q = "".join(rng.choice(list("ACGT"), int(rng.integers(60, 200))))
        a, b = int(rng.integers(0, 30)), int(rng.integers(0, 30))
        t = "".join(rng.choice(list("ACGT"), a)) + t         # the target starts with a stretch the query does not have
        q = q[b:]
        off = int(rng.integers(-6, 7)) if kind != 7 else int(rng.integers(-40, 41))
        if kind == 4 and (it // 8) % 2 == 0:                 # ... and a band that misses the rectangle: score 0
            off += 1000 if rng.random() < 0.5 else -1000
        out.append((t, q, a + b + off))
    return out

"""The CPU statement of window support (sp_pileup_windows_batch, sp_align_pileup_windows_batch) and of the lift-over of a backbone interval onto a consensus
(sp_cyp_variant_windows), as loops over CIGAR ops -- and, to hold these loops themselves to something plainer, a per-column brute force: the alignment expanded to one
character per target column plus the set of junctions that carry an insertion, and a window tested by slicing.

Ops are BAM-encoded words (len << 4 | op): 7 '=', 8 'X', 1 'I' (query only), 2 'D' (target only).  An alignment is (b_start, b_end, a_start, ops)."""

EQ, X, I, D = 7, 8, 1, 2


def op(code, n):
    return (n << 4) | code


def ops_of(text):
    """'10= 1X 2I 3D' -> op words"""
    codes = {"=": EQ, "X": X, "I": I, "D": D}
    return [op(codes[t[-1]], int(t[:-1])) for t in text.split()]


def spans(ops):
    """(target bases, query bases) the ops consume"""
    t = sum(w >> 4 for w in ops if (w & 15) in (EQ, X, D))
    q = sum(w >> 4 for w in ops if (w & 15) in (EQ, X, I))
    return t, q


# ---------------------------------------------------------------------------------------------------------------- window support, by ops
def window_of_pair(b_start, ops, start, end):
    """(span, exact, partial) of one aligned pair for the window [start, end): each 0 or 1"""
    b_end = b_start + spans(ops)[0]
    if not (b_start < end and start < b_end):
        return 0, 0, 0
    if not (b_start <= start and end <= b_end):
        return 0, 0, 1
    exact, t = 1, b_start
    for w in ops:
        code, n = w & 15, w >> 4
        if code == I:
            j = t - 1                                    # the insertion sits between columns j and j + 1
            if start <= j and j + 1 < end:
                exact = 0
        else:
            if code in (X, D) and t < end and start < t + n:
                exact = 0
            t += n
    return 1, exact, 0


def window_support(pairs, alns, windows):
    """pairs: [(query, target)], alns: [(b_start, ops) or None for a pair that did not align], windows: one list of (start, end) per target
    -> one list of (span, exact, partial) per target"""
    out = [[[0, 0, 0] for _ in w] for w in windows]
    for (q, t), aln in zip(pairs, alns):
        if aln is None or not aln[1]:
            continue
        for i, (s, e) in enumerate(windows[t]):
            got = window_of_pair(aln[0], aln[1], s, e)
            for k in range(3):
                out[t][i][k] += got[k]
    return [[tuple(r) for r in w] for w in out]


# ---------------------------------------------------------------------------------------------------------------- the same, by columns
def expand(b_start, ops):
    """(per-column string over '=', 'X', 'D' for columns b_start ..., the set of j such that an insertion sits between columns j and j + 1)"""
    cols, ins, t = [], set(), b_start
    for w in ops:
        code, n = w & 15, w >> 4
        if code == I:
            ins.add(t - 1)
        else:
            cols.append({EQ: "=", X: "X", D: "D"}[code] * n)
            t += n
    return "".join(cols), ins


def window_of_pair_brute(b_start, ops, start, end):
    cols, ins = expand(b_start, ops)
    b_end = b_start + len(cols)
    covered = [c for c in range(start, end) if b_start <= c < b_end]
    if not covered:
        return 0, 0, 0
    if len(covered) != end - start:
        return 0, 0, 1
    inside = cols[start - b_start:end - b_start]
    exact = inside == "=" * (end - start) and not any(j in ins for j in range(start, end - 1))
    return 1, int(exact), 0


# ---------------------------------------------------------------------------------------------------------------- lift-over of [p - F, p + |ref| + F) onto the query
def lift(b_start, a_start, ops, pos, ref_len, flank):
    """the window of a variant on the query, or None: by ops"""
    lo, hi = pos - flank, pos + ref_len + flank
    b_end = b_start + spans(ops)[0]
    if not ops or lo < b_start or hi > b_end:
        return None
    t, q = b_start, a_start
    q_lo = q if t == lo else None
    q_hi = q if t == hi else None
    for w in ops:
        code, n = w & 15, w >> 4
        if code == I:
            q += n
        else:
            on_q = code != D
            if t < lo <= t + n:
                q_lo = q + (lo - t if on_q else 0)
            if t < hi <= t + n:
                q_hi = q + (hi - t if on_q else 0)
            t += n
            q += n if on_q else 0
        if t == hi:
            q_hi = q
    return (q_lo, q_hi) if q_hi > q_lo else None


def lift_brute(b_start, a_start, ops, pos, ref_len, flank):
    """the same from the path written out step by step: states[k] = (target offset, query offset) after k single-base steps"""
    lo, hi = pos - flank, pos + ref_len + flank
    states = [(b_start, a_start)]
    for w in ops:
        code, n = w & 15, w >> 4
        for _ in range(n):
            t, q = states[-1]
            states.append((t + (code != I), q + (code != D)))
    if not ops or lo < b_start or hi > states[-1][0]:
        return None
    q_lo = min(q for t, q in states if t == lo)          # the first time the path stands at lo: before an insertion there
    q_hi = max(q for t, q in states if t == hi)          # the last time it stands at hi: behind one
    return (q_lo, q_hi) if q_hi > q_lo else None


def gt_of(state):
    """the GT of cyp2d6_alleles.vcf.gz for a VariantAlleleRelationship code (0 Unknown, 1 Match, 2 Unexpected, 3 Missing, 4 AmbiguousUnexpected, 5 AmbiguousMissing,
    6 UnknownUnexpected, 7 UnknownMissing; 255 = not listed)"""
    return "." if state in (4, 5) else "1" if state in (1, 2) else "0"

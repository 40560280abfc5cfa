"""A plain statement of the alignment contract of DESIGN.md sections 3.1 and 3.2, written from that text alone: a dictionary and a vote count for the anchor, a
row-by-row dynamic programme over the band for the cell.  It shares no code and no algorithm with oracle/align.c or the HIP kernels (no wavefronts, no
furthest-reaching points), so a mistake the two of them share shows up against it.  Sequences are strings over ACGT; every other character is an N.

    anchor_topk(a, b, k)                     -> k pairs (diagonal, votes), (0, 0) where nothing is left
    cell(a, b, diag, band)                   -> None | ((nm, a_end, b_end), set of the optimal end cells)
    align(a, b, diag, max_ed)                -> None | (nm, a_end, b_end, band used)          the rule of sp_align_batch
    replay(a, b, band, diag, aln, events)    asserts that the events spell an alignment of aln's cost inside the band
"""
import numpy as np

KMER = 16
MAXOCC = 4              # a 16-mer that occurs more often in the indexed sequence does not vote
PEAK_SPREAD = 48        # the anchor is the midpoint of the strongly voted diagonals this close to the peak
PEAK_SUPPRESS = 128     # top-k: the diagonals this close to a taken peak are cleared
BAND, WIDE_BAND = 64, 256
MAX_ED = 511            # the library's cap on the edits of a cell
RETRY_OVER = 32         # sp_align_batch runs the wide band as well when the narrow alignment needed more edits than this
EV_X, EV_D, EV_I = 0, 1, 2
INF = 1 << 28

_CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _i
    _CODE[ord(_c.lower())] = _i


def codes(s):
    """A C G T -> 0 1 2 3, anything else -> 4 (N)"""
    return _CODE[np.frombuffer(s.encode(), np.uint8)] if len(s) else np.zeros(0, np.uint8)


def _is_base(c):
    return c in "ACGTacgt"


# ------------------------------------------------------------------------------------------------ 3.1 anchor
def vote_table(a, b, maxocc=MAXOCC):
    """{d: votes}: every N-free 16-mer of b that occurs 1..maxocc times in a votes for b_pos - a_pos, once per occurrence"""
    a, b = a.upper(), b.upper()
    where = {}
    for p in range(len(a) - KMER + 1):
        w = a[p:p + KMER]
        if all(_is_base(c) for c in w):
            where.setdefault(w, []).append(p)
    votes = {}
    for j in range(len(b) - KMER + 1):
        w = b[j:j + KMER]
        if not all(_is_base(c) for c in w):
            continue
        occ = where.get(w, ())
        if 1 <= len(occ) <= maxocc:
            for p in occ:
                votes[j - p] = votes.get(j - p, 0) + 1
    return votes


def peaks(votes, k):
    votes = dict(votes)
    out = []
    for _ in range(k):
        live = [(v, -d) for d, v in votes.items() if v > 0]
        if not live:
            out.append((0, 0))
            continue
        top, neg = max(live)                               # most votes, ties to the smallest diagonal
        peak = -neg
        need = max(2, top // 8)
        strong = [d for d in range(peak - PEAK_SPREAD, peak + PEAK_SPREAD + 1) if votes.get(d, 0) >= need] + [peak]
        out.append(((min(strong) + max(strong)) // 2, top))
        for d in range(peak - PEAK_SUPPRESS, peak + PEAK_SUPPRESS + 1):
            votes.pop(d, None)
    return out


def anchor_topk(a, b, k):
    if len(a) < KMER or len(b) < KMER:
        return [(0, 0)] * k
    return peaks(vote_table(a, b), k)


# ------------------------------------------------------------------------------------------------ 3.2 cell
def cell(a, b, diag, band=BAND):
    """D[i][j] = fewest edits of an alignment that starts for free at the first in-rectangle cell of a band diagonal and has consumed a[:i] and b[:j], over the cells
    with diag - band/2 <= j - i <= diag + band/2 - 1.  A row is held by lane: lane l of row i is the cell j = i + (diag - band/2) + l, so the diagonal step comes
    from the same lane of the row above, the step that consumes a base of A from lane l + 1 of the row above, and the step that consumes a base of B from lane
    l - 1 of the same row (a running minimum)."""
    A, B = codes(a), codes(b)
    m, n = len(A), len(B)
    if m == 0 or n == 0:
        return None
    kbase = diag - band // 2
    lanes = np.arange(band)
    # b's codes with a margin of N on both sides: the B base under lane l of row i is bp[i + off + l]
    off = band + m + 1
    bp = np.full(n + 2 * off + band, 4, np.uint8)
    bp[off:off + n] = B
    ends = {}                                              # (i, j) -> D for the band cells on the last row or the last column

    def valid_range(i):
        lo, hi = max(0, -i - kbase), min(band - 1, n - i - kbase)
        return lo, hi

    # row 0: every band diagonal that starts on it, and the cells right of them at one edit per base of B
    lo, hi = valid_range(0)
    prev = np.full(band, INF, np.int64)
    if lo <= hi:
        j = kbase + lanes
        prev[lo:hi + 1] = np.where(j[lo:hi + 1] < n, 0, INF)
        prev = np.minimum.accumulate(prev - lanes) + lanes
        prev[:lo] = INF
        prev[hi + 1:] = INF
        prev[prev > INF] = INF
        if kbase + hi == n:
            ends[(0, n)] = int(prev[hi])
    # the rows that hold a band cell at all: 0 <= i + kbase + l <= n for some lane (the rows before and behind them are empty)
    first, last = max(1, 1 - band - kbase), min(m, n - kbase)
    if first > 1 or last < first:
        prev = np.full(band, INF, np.int64)
    for i in range(first, last + 1):
        lo, hi = valid_range(i)
        row = np.full(band, INF, np.int64)
        if lo <= hi:
            x = A[i - 1]
            under = bp[off + i - 1 + kbase:off + i - 1 + kbase + band]          # b[j - 1] for j = i + kbase + l
            sub = np.ones(band, np.int64) if x > 3 else ((under != x) | (under > 3)).astype(np.int64)
            t = prev + sub
            t[:-1] = np.minimum(t[:-1], prev[1:] + 1)
            if i < m and i + kbase + lo == 0 and n > 0:    # the diagonal that starts on the first column at this row
                t[lo] = 0
            t[:lo] = INF
            t[hi + 1:] = INF
            row = np.minimum.accumulate(t - lanes) + lanes
            row[:lo] = INF
            row[hi + 1:] = INF
            row[row > INF] = INF
            if i < m and i + kbase + hi == n:
                ends[(i, n)] = int(row[hi])
        prev = row
    lo, hi = valid_range(m)
    for l in range(lo, hi + 1):
        ends[(m, m + kbase + l)] = int(prev[l])
    ends = {c: d for c, d in ends.items() if d < INF}
    if not ends:
        return None
    nm = min(ends.values())
    best = frozenset(c for c, d in ends.items() if d == nm)

    def order(c):                                         # longest path, then the lane nearest band / 2, then the lowest lane
        l = c[1] - c[0] - kbase
        return (c[0] + c[1], -abs(l - band // 2), -l)
    e = max(best, key=order)
    return (nm, e[0], e[1]), best


def align(a, b, diag, max_ed, run_cell=cell):
    """sp_align_batch: 64 diagonals; 256 as well when that is lost or needed more than 32 edits; the wide result when the narrow one is lost or the wide one has
    strictly fewer edits.  (run_cell: cell, or a memo of it)"""
    cap = min(max_ed, MAX_ED)

    def run(band):
        r = run_cell(a, b, diag, band)
        return None if r is None or r[0][0] > cap else r[0]
    narrow = run(BAND)
    if narrow is not None and narrow[0] <= RETRY_OVER:
        return narrow + (BAND,)
    wide = run(WIDE_BAND)
    if wide is not None and (narrow is None or wide[0] < narrow[0]):
        return wide + (WIDE_BAND,)
    return None if narrow is None else narrow + (BAND,)


def full_matrix(a, b):
    """the same ends-free unit-cost programme over the whole rectangle, one cell at a time (the self-check of cell() where the band covers everything)"""
    m, n = len(a), len(b)
    if m == 0 or n == 0:
        return None
    D = [[INF] * (n + 1) for _ in range(m + 1)]
    for i in range(m + 1):
        for j in range(n + 1):
            best = 0 if ((i == 0 or j == 0) and i < m and j < n) else INF
            if i > 0 and j > 0:
                same = a[i - 1] == b[j - 1] and _is_base(a[i - 1])
                best = min(best, D[i - 1][j - 1] + (0 if same else 1))
            if j > 0:
                best = min(best, D[i][j - 1] + 1)
            if i > 0:
                best = min(best, D[i - 1][j] + 1)
            D[i][j] = best
    ends = {(i, j): D[i][j] for i in range(m + 1) for j in range(n + 1) if i == m or j == n}
    nm = min(ends.values())
    return nm, {c for c, d in ends.items() if d == nm}


def anchor_bruteforce(a, b, k):
    """anchor_topk by a double loop over positions (no dictionary)"""
    m, n = len(a), len(b)
    if m < KMER or n < KMER:
        return [(0, 0)] * k
    clean = lambda w: all(_is_base(c) for c in w)
    votes = {}
    for j in range(n - KMER + 1):
        w = b[j:j + KMER]
        if not clean(w):
            continue
        hits = [p for p in range(m - KMER + 1) if a[p:p + KMER] == w]
        if 1 <= len(hits) <= MAXOCC:
            for p in hits:
                votes[j - p] = votes.get(j - p, 0) + 1
    return peaks(votes, k)


# ------------------------------------------------------------------------------------------------ events
def replay(a, b, band, diag, aln, events):
    """aln = (nm, a_start, a_end, b_start, b_end); events = the event words (type << 30 | b_pos) in path order.  Asserts that they spell an alignment: it starts
    where a band diagonal enters the rectangle, every base outside an event is an exact N-free match, X sits on a true mismatch or an N, every visited cell is in
    the band, it ends at (a_end, b_end) on the last row or column, and it has nm events."""
    nm, a_start, a_end, b_start, b_end = (int(x) for x in aln)
    m, n = len(a), len(b)
    lo, hi = diag - band // 2, diag + band // 2 - 1
    i, j = a_start, b_start
    assert (i == 0 or j == 0) and 0 <= i < m and 0 <= j < n, ("start", i, j)
    assert lo <= j - i <= hi, ("start outside the band", i, j)
    assert len(events) == nm, ("events", len(events), nm)

    def match_to(stop_j=None, stop_i=None):
        nonlocal i, j
        while (stop_j is not None and j < stop_j) or (stop_i is not None and i < stop_i):
            assert i < m and j < n, ("match runs out of the rectangle", i, j)
            assert a[i].upper() == b[j].upper() and _is_base(a[i]), ("not a match", i, j, a[i], b[j])
            i += 1
            j += 1
    for e in events:
        e = int(e)
        kind, bpos = e >> 30, e & 0x3FFFFFFF
        assert kind in (EV_X, EV_D, EV_I), e
        assert bpos >= j, ("event behind the path", bpos, j)
        match_to(stop_j=bpos)
        if kind == EV_X:
            assert i < m and j < n, ("X outside", i, j)
            assert not (a[i].upper() == b[j].upper() and _is_base(a[i])), ("X on a match", i, j)
            i += 1
            j += 1
        elif kind == EV_D:
            assert j < n, ("D outside", i, j)
            j += 1
        else:
            assert i < m, ("I outside", i, j)
            i += 1
        assert lo <= j - i <= hi, ("outside the band", i, j)
    match_to(stop_i=a_end)
    assert (i, j) == (a_end, b_end), ("end", (i, j), (a_end, b_end))
    assert i == m or j == n, ("end is not on the last row or column", i, j)

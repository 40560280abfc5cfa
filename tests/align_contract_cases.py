"""Designed cases for the anchor and the unit-cost cell: each family aims at one place where the hand-written device paths change over, at the
smallest shape that reaches it, and each case's name says which.  Everything is built from seeded numpy; the expected values come from
tests/align_contract_ref.py, never from the code under test.

    cell_families()    {family: [Cell]}     Cell = (name, a, b, diag, max_ed, may_lose)
    anchor_families()  {family: [Anchor]}   Anchor = (name, a, b)            a is the indexed side, diagonal = b_pos - a_pos

A family is uploaded as its own pair of sets, so the LDS slot, the N planes and the vote bins are sized by the family.  may_lose marks the only cases for which
the reference may report no alignment under sp_align_batch's rule: a band that misses the rectangle, a drift that no band tried holds, an edit cap below the cost.
"""
import functools
from collections import namedtuple

import numpy as np

import align_contract_ref as ref

Cell = namedtuple("Cell", "name a b diag max_ed may_lose")
Anchor = namedtuple("Anchor", "name a b")


def rseq(rng, n):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, n))


def other(rng, c):
    return "ACGT"[("ACGT".index(c) + 1 + int(rng.integers(3))) % 4] if c in "ACGT" else "A"


def sub_at(rng, s, positions):
    s = list(s)
    for p in positions:
        s[p] = other(rng, s[p])
    return "".join(s)


def put(s, p, c):
    return s[:p] + c + s[p + 1:]


@functools.lru_cache(maxsize=None)
def ref_cell(a, b, diag, band):
    """ref.cell, computed once per process and left unchanged"""
    return ref.cell(a, b, diag, band)


def ref_align(case):
    return ref.align(case.a, case.b, case.diag, case.max_ed, run_cell=ref_cell)


@functools.lru_cache(maxsize=None)
def ref_anchor(a, b, k):
    return tuple(ref.anchor_topk(a, b, k))


# ================================================================================================ cell families
EDGE_LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65)


def fam_lengths():
    """every pair of the lengths around the 16-base compare and the 64-lane band, the shorter sequence contained in the longer (equal: one substitution), and
    dovetails in both directions"""
    rng = np.random.default_rng(4101)
    out = []
    for la in EDGE_LENGTHS:
        for lb in EDGE_LENGTHS:
            if la == lb:
                a = rseq(rng, la)
                b = sub_at(rng, a, [la // 2]) if la > 2 else a
                out.append(Cell(f"len_equal_{la}", a, b, 0, 255, False))
            elif la < lb:
                b = rseq(rng, lb)
                at = int(rng.integers(0, lb - la + 1))
                out.append(Cell(f"len_a{la}_in_b{lb}_at{at}", b[at:at + la], b, at, 255, False))
            else:
                a = rseq(rng, la)
                at = int(rng.integers(0, la - lb + 1))
                out.append(Cell(f"len_b{lb}_in_a{la}_at{at}", a, a[at:at + lb], -at, 255, False))
    for ln in EDGE_LENGTHS:
        ov = (ln + 1) // 2
        g = rseq(rng, 2 * ln - ov)
        out.append(Cell(f"len_dovetail_a_end_b_start_{ln}", g[:ln], g[ln - ov:], -(ln - ov), 255, False))
        out.append(Cell(f"len_dovetail_b_end_a_start_{ln}", g[ln - ov:], g[:ln], ln - ov, 255, False))
    return out


STRETCHES = (15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 2047, 2048, 2049)


def _stretch_pair(rng, off, stretch, flank_b=0):
    """a clean stretch of exactly `stretch` bases between two substitutions, starting at offset `off` of one of A's 16-base blocks"""
    pre = 16 + off - 1                                      # the first substitution sits just before the stretch
    a = rseq(rng, pre + 1 + stretch + 1 + 20)
    b = sub_at(rng, a, [pre, pre + 1 + stretch])
    return a, rseq(rng, flank_b) + b


def fam_handover():
    """the hand-over of a lane that matched 16 bases to the cooperative step, and the 1,024-base step itself: a clean stretch of each critical length at every
    offset of A's 16-base blocks"""
    rng = np.random.default_rng(4102)
    out = []
    for stretch in STRETCHES:
        for off in range(16):
            fl = (0, 5, 16, 37)[off % 4]
            a, b = _stretch_pair(rng, off, stretch, fl)
            out.append(Cell(f"stretch_{stretch}_off{off}_flank{fl}", a, b, fl, 255, False))
    return out


def fam_kept_scan():
    """two and three substitutions on one diagonal inside one 1,024-base span (the kept scan answers the later stretches), and an indel in between (the path
    moves to the neighbouring diagonal: the kept scan must not be used)"""
    rng = np.random.default_rng(4103)
    out = []
    for off in range(16):
        start = 16 + off
        a = rseq(rng, start + 1000)
        two = [start - 1, start + 200, start + 450]
        three = two + [start + 700]
        out.append(Cell(f"kept_two_stretches_off{off}", a, sub_at(rng, a, two), 0, 255, False))
        out.append(Cell(f"kept_three_stretches_off{off}", a, rseq(rng, 9) + sub_at(rng, a, three), 9, 255, False))
        # substitution, 200 clean, an indel, 200 clean, substitution, 200 clean
        s = sub_at(rng, a, [start - 1, start + 400])
        ins = s[:start + 200] + rseq(rng, 1 + off % 3) + s[start + 200:]
        dele = s[:start + 200] + s[start + 200 + 1 + off % 3:]
        out.append(Cell(f"kept_scan_then_insertion_off{off}", a, ins, 0, 255, False))
        out.append(Cell(f"kept_scan_then_deletion_off{off}", a, dele, 0, 255, False))
    return out


def _fam_scan_n(where, seed):
    rng = np.random.default_rng(seed)
    out = []
    for off in (0, 7, 15):
        for npos in (3, 16, 31, 300, 1023, 1040):           # inside the first 16-base compare, at block edges, inside and behind the first cooperative step
            start = 16 + off
            a = rseq(rng, start + 1300)
            b = sub_at(rng, a, [start - 1, start + 1200])
            if where in ("a", "both"):
                a = put(a, start + npos, "N")
            if where in ("b", "both"):
                b = put(b, start + npos + (5 if where == "both" else 0), "N")
            out.append(Cell(f"scan_n_in_{where}_off{off}_at{npos}", a, b, 0, 255, False))
    return out


def fam_scan_n_in_a():
    """an N inside the scanned span, in A only: A's set carries an N plane, B's set has none"""
    return _fam_scan_n("a", 4104)


def fam_scan_n_in_b():
    """the same with the N in B only: B's set carries the N plane, A's has none"""
    return _fam_scan_n("b", 4105)


def fam_scan_n_both():
    return _fam_scan_n("both", 4106)


def _drift_pair(rng, drift, pieces):
    """b drifts `drift` diagonals away from a between two clean blocks of 400 bases: drift > 0 inserts into b (D events), drift < 0 into a (I events); in
    `pieces` indels 40 bases apart"""
    sizes = [abs(drift) // pieces + (1 if x < abs(drift) % pieces else 0) for x in range(pieces)]
    core = rseq(rng, 800 + 40 * pieces)
    plain, gapped, at = core, "", 400
    last = 0
    for x, size in enumerate(sizes):
        gapped += core[last:at] + rseq(rng, size)
        last = at
        at += 40
    gapped += core[last:]
    return (plain, gapped) if drift > 0 else (gapped, plain)


def fam_band_edges():
    """the band's first and last lane: a net drift of exactly 30..33 diagonals (64) and 126..129 (256) in both directions, by one indel and by several; the anchor
    handed in off-centre; a band that misses the rectangle; a diagonal so far out that one lane alone starts inside it"""
    rng = np.random.default_rng(4107)
    out = []
    for mag in (30, 31, 32, 33, 126, 127, 128, 129):
        for sign in (1, -1):
            drift = sign * mag
            # the widest band tried holds diagonals diag - 128 .. diag + 127: a drift beyond that is out of reach
            lose = drift > 127 or drift < -128
            for pieces in (1, 5):
                a, b = _drift_pair(rng, drift, pieces)
                out.append(Cell(f"drift_{drift:+d}_in_{pieces}_indels", a, b, 0, 140, lose))      # (140: mismatching through a clean block instead costs more)
    a = rseq(rng, 300)
    b = rseq(rng, 50) + sub_at(rng, a, [100, 200]) + rseq(rng, 50)
    for shift in (-32, -31, 0, 31, 32):
        out.append(Cell(f"anchor_off_centre_{shift:+d}", a, b, 50 + shift, 255, False))
    a, b = rseq(rng, 120), rseq(rng, 150)
    for diag in (150 + 200, -120 - 200, 150 + 33, -120 - 32):
        out.append(Cell(f"band_misses_rectangle_diag{diag:+d}", a, b, diag, 255, True))
    out.append(Cell("only_lane_0_starts_inside", a, b, 150 + 31, 255, False))
    out.append(Cell("only_lane_63_starts_inside", a, b, -120 - 30, 255, False))
    out.append(Cell("only_lane_0_starts_inside_match", a, b[:-1] + a[0], 150 + 31, 255, False))
    out.append(Cell("only_lane_63_starts_inside_match", a[:-1] + b[0], b, -120 - 30, 255, False))
    return out


def end_tie_kind(a, b, diag, band=64):
    """which rule of the end order the pair needs: None (one optimal end cell), 'path' (the cells differ in i + j), 'central' (the longest ones differ in their
    distance from lane band / 2), 'lowest' (two of the longest are equally central)"""
    r = ref.cell(a, b, diag, band)
    if r is None or len(r[1]) < 2:
        return None
    cells = sorted(r[1], key=lambda c: -(c[0] + c[1]))
    longest = [c for c in cells if c[0] + c[1] == cells[0][0] + cells[0][1]]
    if len(longest) == 1:
        return "path"
    dist = sorted(abs(c[1] - c[0] - diag) for c in longest)          # lane - band / 2 = (j - i) - diag
    return "lowest" if dist[0] == dist[1] else "central"


@functools.lru_cache(maxsize=None)
def fam_end_ties():
    """pairs whose optimum reaches the last row or column on several diagonals at the same cost: a trailing homopolymer or tandem repeat in B behind A's end, and
    a seeded search over short two-letter pairs that keeps the first eight that need each rule of the end order (the reference names the rule)"""
    rng = np.random.default_rng(4108)
    out = []
    r = rseq(rng, 40)
    out.append(Cell("tie_homopolymer_tail", r + "A" * 6, r + "A" * 3 + "G" + "A" * 12 + rseq(rng, 10), 0, 255, False))
    out.append(Cell("tie_tandem_tail", "AC" * 12, "G" + "AC" * 20 + rseq(rng, 10), 5, 255, False))
    out.append(Cell("tie_homopolymer_both", "A" * 20, "A" * 40, 10, 255, False))
    out.append(Cell("tie_homopolymer_square", "A" * 24 + "C", "A" * 24 + "G", 0, 255, False))
    kept = {"path": 0, "central": 0, "lowest": 0}
    for t in range(4000):
        if min(kept.values()) >= 8:
            break
        la, lb = int(rng.integers(2, 15)), int(rng.integers(2, 15))
        a = "".join("AC"[x] for x in rng.integers(0, 2, la))
        b = "".join("AC"[x] for x in rng.integers(0, 2, lb))
        diag = int(rng.integers(-6, 7))
        kind = end_tie_kind(a, b, diag)
        if kind is not None and kept[kind] < 8:
            kept[kind] += 1
            out.append(Cell(f"tie_{kind}_{kept[kind]}", a, b, diag, 255, False))
    return out


@functools.lru_cache(maxsize=None)
def edit_cap_pairs():
    """(a at 511 edits, b, a at 512 edits, b): substitutions are added to a 1,200-base sequence until the reference needs exactly that many edits on 256 diagonals
    (which hold the 64: the wide cost is the smaller one).  One more substitution moves the cost by at most one, so adding (target - cost) never overshoots."""
    rng = np.random.default_rng(4109)
    b = rseq(rng, 1200)
    order = [int(x) for x in rng.permutation(1200)]
    repl = [other(rng, b[p]) for p in order]
    found = {}
    used = 0
    for target in (511, 512):
        while True:
            a = list(b)
            for p, c in zip(order[:used], repl[:used]):
                a[p] = c
            a = "".join(a)
            nm = ref.cell(a, b, 0, 256)[0][0]
            if nm == target:
                found[target] = a
                break
            assert nm < target and used < 1200, (nm, target, used)
            used += target - nm
    return found[511], b, found[512], b


@functools.lru_cache(maxsize=None)
def fam_caps():
    """the edit cap at the cost, one below it and at 0; the second try on 256 diagonals after more than 32 edits on 64, once strictly cheaper and once not; the
    library's cap of 511 edits met exactly and missed by one"""
    rng = np.random.default_rng(4110)
    out = []
    a = rseq(rng, 400)
    pairs = [("subs", a, rseq(rng, 20) + sub_at(rng, a, [30, 90, 91, 200, 333]), 20)]
    e = sub_at(rng, a, [50, 300])
    pairs.append(("indels", a, e[:120] + rseq(rng, 4) + e[120:250] + e[253:], 0))
    for name, x, y, diag in pairs:
        nm = ref.align(x, y, diag, 511)[0]
        assert nm >= 2
        out.append(Cell(f"cap_at_cost_{name}_nm{nm}", x, y, diag, nm, False))
        out.append(Cell(f"cap_below_cost_{name}_nm{nm}", x, y, diag, nm - 1, True))
        out.append(Cell(f"cap_zero_{name}", x, y, diag, 0, True))
    out.append(Cell("cap_zero_identical", a, a, 0, 0, False))
    # more than 32 edits on 64 diagonals: an insertion of 40 bases with 90 bases behind it (64 diagonals pay mismatches to the end, 256 pay the 40)
    x = rseq(rng, 500)
    out.append(Cell("retry2_wide_strictly_cheaper", x, x[:410] + rseq(rng, 40) + x[410:], 0, 255, False))
    out.append(Cell("retry2_wide_not_cheaper", x, sub_at(rng, x, range(5, 485, 12)), 0, 255, False))
    a511, b, a512, _ = edit_cap_pairs()
    out.append(Cell("cap_511_edits_exactly", a511, b, 0, 511, False))
    out.append(Cell("cap_512_edits_lost", a512, b, 0, 511, True))
    return out


SLOT_SHORT = (16, 17, 31, 32, 33, 40)
SLOT_LONG = (2992, 2993, 3000, 3007)          # 0, 1, 8 and 15 modulo 16


def _fam_slot(short_is_a, seed):
    rng = np.random.default_rng(seed)
    out = []
    for x, ls in enumerate(SLOT_SHORT):
        for y, ll in enumerate(SLOT_LONG):
            long_ = rseq(rng, ll)
            for where, at in (("first64", (x * 7 + y) % (64 - 40)), ("last64", ll - ls - (x + 3 * y) % 24), ("middle", 1000 + 16 * y + x)):
                short = long_[at:at + ls]
                if ls > 20:
                    short = sub_at(rng, short, [ls // 2])
                if short_is_a:
                    out.append(Cell(f"slot_a{ls}_b{ll}_{where}", short, long_, at, 255, False))
                else:
                    out.append(Cell(f"slot_a{ll}_b{ls}_{where}", long_, short, -at, 255, False))
    return out


def fam_slot_short_a():
    """sets whose longest sequences differ widely (the LDS slot is sized by the shorter set): A of at most 40 bases against B of 3,000, the hit in B's first and
    last 64 bases and in the middle, lengths 0, 1 and 15 modulo 16 on both sides"""
    return _fam_slot(True, 4111)


def fam_slot_short_b():
    """the reverse: A of 3,000 bases against B of at most 40"""
    return _fam_slot(False, 4112)


FUZZ_LENGTHS = (5, 17, 40, 90, 200, 400, 1100)


def fam_fuzz():
    """300 seeded pairs: up to 8 edits, each a substitution (N included), an insertion or a deletion of 1..40 bases; flanks of 0..50 bases; the diagonal handed in
    within +-60 of the true one"""
    rng = np.random.default_rng(4113)
    out = []
    for x in range(300):
        ln = int(rng.choice(FUZZ_LENGTHS))
        a = rseq(rng, ln)
        s = list(a)
        for _ in range(int(rng.integers(0, 9))):
            kind = int(rng.integers(0, 3))
            if kind == 0 and s:
                p = int(rng.integers(0, len(s)))
                s[p] = "ACGTN"[int(rng.integers(0, 5))]
            elif kind == 1:
                p = int(rng.integers(0, len(s) + 1))
                s[p:p] = list(rseq(rng, int(rng.integers(1, 41))))
            elif len(s) > 1:
                size = int(rng.integers(1, 41))
                p = int(rng.integers(0, len(s)))
                del s[p:p + min(size, len(s) - 1)]
        left, right = int(rng.integers(0, 51)), int(rng.integers(0, 51))
        b = rseq(rng, left) + "".join(s) + rseq(rng, right)
        if rng.integers(0, 8) == 0:
            a = put(a, int(rng.integers(0, ln)), "N")
        out.append(Cell(f"fuzz_{x}_len{ln}", a, b, left + int(rng.integers(-60, 61)), 255, True))
    return out


@functools.lru_cache(maxsize=None)
def cell_families():
    fams = dict(lengths=fam_lengths(), handover=fam_handover(), kept_scan=fam_kept_scan(), scan_n_in_a=fam_scan_n_in_a(), scan_n_in_b=fam_scan_n_in_b(),
                scan_n_both=fam_scan_n_both(), band_edges=fam_band_edges(), end_ties=fam_end_ties(), caps=fam_caps(), slot_short_a=fam_slot_short_a(),
                slot_short_b=fam_slot_short_b(), fuzz=fam_fuzz())
    for name, cases in fams.items():
        assert len({c.name for c in cases}) == len(cases), name
    return fams


# ================================================================================================ anchor families
def _shifted(rng, shared, shift, pad=60):
    """(a, b) that share `shared` on diagonal `shift` and nothing else"""
    return rseq(rng, pad + max(0, -shift)) + shared + rseq(rng, pad), rseq(rng, pad + max(0, shift)) + shared + rseq(rng, pad)


def _two_segments(rng, votes1, votes2, delta):
    """(a, b): a segment that gives votes1 votes on diagonal 0 and one that gives votes2 on diagonal delta"""
    u, v = rseq(rng, votes1 + 15), rseq(rng, votes2 + 15)
    junk = rseq(rng, abs(delta))
    return (u + v, u + junk + v) if delta > 0 else (u + junk + v, u + v)


def afam_occurrences():
    """a 16-mer that occurs exactly 4 times in A votes, one that occurs 5 times does not (SP_MAXOCC)"""
    rng = np.random.default_rng(4201)
    out = []
    kmer = rseq(rng, 16)
    for occ in (1, 4, 5):
        # (the bases beside the 16-mer differ between the two sides: no window that only overlaps it is shared)
        a = "".join(rseq(rng, 150 + 11 * x) + "A" + kmer + "A" for x in range(occ)) + rseq(rng, 30)
        out.append(Anchor(f"kmer_occurs_{occ}_times_alone", a, rseq(rng, 40) + "C" + kmer + "C" + rseq(rng, 40)))
        seg = rseq(rng, 24)                                  # and beside a unique segment of 9 votes
        out.append(Anchor(f"kmer_occurs_{occ}_times_beside_unique", a + "G" + seg + "G" + rseq(rng, 20),
                          rseq(rng, 40) + "C" + kmer + "C" + rseq(rng, 40) + "T" + seg))
    return out


def afam_n_windows():
    """an N kills exactly the 16 windows over it, on either side; at the first and last base it kills one"""
    rng = np.random.default_rng(4202)
    out = []
    s = rseq(rng, 200)
    for pos in (0, 1, 15, 16, 100, 184, 185, 199):
        out.append(Anchor(f"n_in_looked_up_at{pos}", rseq(rng, 7) + s, put(s, pos, "N")))
        out.append(Anchor(f"n_in_indexed_at{pos}", put(s, pos, "N"), rseq(rng, 7) + s))
    out.append(Anchor("n_every_16th_no_window", s, "".join("N" if p % 16 == 15 else c for p, c in enumerate(s))))
    return out


def afam_lookups():
    """len - 15 = 511 .. 513 and 1,023 .. 1,025 looked-up 16-mers (512 threads x 2 look-ups), and one clean diagonal of 64 k +- 1 votes (runs of equal votes that
    end at a wave's edge)"""
    rng = np.random.default_rng(4203)
    out = []
    for windows in (511, 512, 513, 1023, 1024, 1025):
        b = rseq(rng, windows + 15)
        out.append(Anchor(f"lookups_{windows}", rseq(rng, 30) + b + rseq(rng, 11), b))
    for votes in (63, 64, 65, 127, 129, 191, 193, 511, 513):
        seg = rseq(rng, votes + 15)
        out.append(Anchor(f"clean_diagonal_{votes}_votes", seg, seg))
        a, b = _shifted(rng, seg, 23 - votes % 7, pad=int(rng.integers(1, 64)))
        out.append(Anchor(f"clean_diagonal_{votes}_votes_offset", a, b))
    return out


def afam_buckets():
    """codes in the first and the last bucket of the table: 16-mers that begin and end with AAAAA / TTTTT"""
    rng = np.random.default_rng(4204)
    out = []
    for base in "AT":
        seg = rseq(rng, 20) + base * 5 + rseq(rng, 6) + base * 5 + rseq(rng, 20)
        for shift in (-17, 40):
            a, b = _shifted(rng, seg, shift)
            out.append(Anchor(f"bucket_poly{base}_shift{shift:+d}", a, b))
        out.append(Anchor(f"bucket_poly{base}_only", base * 5 + "CG" * 3 + base * 5 + rseq(rng, 3), rseq(rng, 3) + base * 5 + "CG" * 3 + base * 5))
        out.append(Anchor(f"bucket_homopolymer_{base}_over_maxocc", base * 40, base * 40))
        out.append(Anchor(f"bucket_homopolymer_{base}_at_maxocc", base * 19, base * 16))
    return out


def afam_extreme_diagonals():
    """the peak on the smallest and on the largest possible diagonal, with len(A) + len(B) + 1 both odd and even (the last bin in either half of a packed dword)"""
    rng = np.random.default_rng(4205)
    out = []
    for la, lb in ((100, 101), (100, 100), (77, 40), (16, 51), (50, 16)):
        k1, k2 = rseq(rng, 16), rseq(rng, 16)
        out.append(Anchor(f"peak_smallest_diagonal_a{la}_b{lb}", rseq(rng, la - 16) + k1, k1 + rseq(rng, lb - 16)))
        out.append(Anchor(f"peak_largest_diagonal_a{la}_b{lb}", k2 + rseq(rng, la - 16), rseq(rng, lb - 16) + k2))
        out.append(Anchor(f"peak_both_extremes_a{la}_b{lb}", k2 + rseq(rng, la - 32) + k1 if la >= 32 else k2, k1 + rseq(rng, lb - 32) + k2 if lb >= 32 else k2))
    return out


def afam_peaks():
    """vote ties between two diagonals; a split peak for the midpoint rule (the second diagonal at +-48 and +-49, holding exactly peak / 8 votes and one fewer);
    top-4 with a second peak at +-128 and +-129 of the first, and fewer peaks than asked for"""
    rng = np.random.default_rng(4206)
    out = []
    for delta in (-300, -49, -48, -20, 20, 48, 49, 300):
        a, b = _two_segments(rng, 25, 25, delta)
        out.append(Anchor(f"tie_two_diagonals_{delta:+d}", a, b))
    for peak in (80, 87, 88, 15, 16, 24):
        need = max(2, peak // 8)
        for delta in (-49, -48, 48, 49):
            for second in (need, need - 1):
                a, b = _two_segments(rng, peak, second, delta)
                out.append(Anchor(f"split_peak{peak}_second{second}_at{delta:+d}", a, b))
    for delta in (-129, -128, 128, 129):
        a, b = _two_segments(rng, 60, 30, delta)
        out.append(Anchor(f"top4_second_peak_at{delta:+d}", a, b))
    u, v, w = rseq(rng, 60), rseq(rng, 50), rseq(rng, 40)
    out.append(Anchor("top4_three_peaks", u + v + w, w + rseq(rng, 200) + v + rseq(rng, 333) + u))
    g = [rseq(rng, 30 + 3 * x) for x in range(5)]
    out.append(Anchor("top4_five_peaks", "".join(g), "".join(s + rseq(rng, 300 + 17 * x) for x, s in enumerate(reversed(g)))))
    out.append(Anchor("top4_no_peak", rseq(rng, 200), rseq(rng, 300)))
    return out


def afam_short():
    """sequences of 15 and 16 bases"""
    rng = np.random.default_rng(4207)
    k = rseq(rng, 16)
    return [Anchor("a15_b40", k[:15], k[:15] + rseq(rng, 25)), Anchor("a40_b15", k[:15] + rseq(rng, 25), k[:15]), Anchor("a16_b16_equal", k, k),
            Anchor("a16_b16_differ", k, other(rng, k[0]) + k[1:]), Anchor("a16_in_b40", k, rseq(rng, 13) + k + rseq(rng, 11)),
            Anchor("b16_in_a40", rseq(rng, 13) + k + rseq(rng, 11), k), Anchor("a15_b15", k[:15], k[:15])]


def afam_global_table():
    """A of 16,500 bases against B of 600: A's table no longer fits in LDS beside the vote bins and is searched in global memory"""
    rng = np.random.default_rng(4208)
    a = rseq(rng, 16500)
    b = sub_at(rng, a[7000:7600], [100, 250, 251, 599])
    return [Anchor("a16500_b600_table_in_global_memory", a, b), Anchor("a16500_b600_at_the_end", a, rseq(rng, 40) + a[-560:]),
            Anchor("a16500_b600_split", a, a[100:400] + rseq(rng, 30) + a[400:670])]


@functools.lru_cache(maxsize=None)
def anchor_families():
    fams = dict(occurrences=afam_occurrences(), n_windows=afam_n_windows(), lookups=afam_lookups(), buckets=afam_buckets(),
                extreme_diagonals=afam_extreme_diagonals(), peaks=afam_peaks(), short=afam_short(), global_table=afam_global_table())
    for name, cases in fams.items():
        assert len({c.name for c in cases}) == len(cases), name
    return fams

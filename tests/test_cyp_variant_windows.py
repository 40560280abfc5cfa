"""sp_cyp_variant_windows (host only): the window of a database variant on a consensus, from the alignment of the consensus (query) onto the backbone (target),
held to tests/pileup_win_ref.py on designed CIGARs -- and that reference to its own step-by-step brute force.

The rule: variant at p with |ref| bases and flank F owns the backbone interval [p - F, p + |ref| + F); covered iff it lies inside [b_start, b_end); its window is
[q_lo, q_hi) with q_lo taken BEFORE an insertion at the left junction and q_hi AFTER one at the right junction; an empty window is none."""
import numpy as np
import pytest

import pileup_win_ref as ref

B_START, A_START = 100, 7
# name -> ops; the backbone span is [100, 100 + target bases)
CIGARS = {
    "clean": "200=",
    "ins_inside": "60= 3I 140=",
    "ins_and_del": "40= 2I 20= 5D 30= 1X 10= 4I 94=",
    "del_long": "50= 30D 120=",
    "mixed": "10= 1X 9= 2D 20= 6I 30= 1D 1I 40= 12D 75=",
}
FLANKS = (0, 2, 8)
REF_LENS = (0, 1, 5)


def aln_of(ffi, ops):
    tl, ql = ref.spans(ops)
    a = np.zeros(1, ffi.AFFINE_DTYPE)
    a[0] = (1, 0, A_START, A_START + ql, B_START, B_START + tl)
    return a


def test_the_reference_agrees_with_its_brute_force():
    n = 0
    for text in CIGARS.values():
        ops = ref.ops_of(text)
        b_end = B_START + ref.spans(ops)[0]
        for F in FLANKS:
            for rl in REF_LENS:
                for p in range(B_START - 3, b_end + 3):
                    assert ref.lift(B_START, A_START, ops, p, rl, F) == ref.lift_brute(B_START, A_START, ops, p, rl, F), (text, F, rl, p)
                    n += 1
    assert n > 9000


@pytest.mark.parametrize("name", sorted(CIGARS))
@pytest.mark.parametrize("flank", FLANKS)
def test_every_position_of_every_designed_cigar(pkg, name, flank):
    ops = ref.ops_of(CIGARS[name])
    b_end = B_START + ref.spans(ops)[0]
    pos, rl = [], []
    for r in REF_LENS:
        for p in range(B_START - 3, b_end + 3):
            pos.append(p)
            rl.append(r)
    got = pkg.database.cyp_variant_windows(aln_of(pkg.ffi, ops), ops, pos, rl, flank)
    want = [ref.lift(B_START, A_START, ops, p, r, flank) for p, r in zip(pos, rl)]
    assert got == want
    assert any(w is None for w in want) and any(w is not None for w in want)


def test_the_designed_edges(pkg):
    db, ffi = pkg.database, pkg.ffi
    one = lambda text, p, rl, F: db.cyp_variant_windows(aln_of(ffi, ref.ops_of(text)), ref.ops_of(text), [p], [rl], F)[0]
    q = lambda t: A_START + (t - B_START)                                   # the query offset of backbone position t on a clean alignment
    # a clean alignment: the interval itself, shifted
    assert one("200=", 150, 1, 2) == (q(148), q(153))
    # touching b_start / b_end exactly is covered, one base beyond is not
    assert one("200=", 102, 1, 2) == (q(100), q(105)) and one("200=", 101, 1, 2) is None
    assert one("200=", 297, 1, 2) == (q(295), q(300)) and one("200=", 298, 1, 2) is None
    assert one("200=", 100, 5, 0) == (q(100), q(105)) and one("200=", 295, 5, 0) == (q(295), q(300)) and one("200=", 296, 5, 0) is None
    # "60= 3I 140=": the insertion sits at the junction in front of backbone position 160, query offsets 67..69
    ins = "60= 3I 140="
    assert one(ins, 162, 1, 2) == (A_START + 60, A_START + 63 + 5)          # exactly at the left edge junction: q_lo in front of it, the inserted bases inside
    assert one(ins, 157, 1, 2) == (A_START + 55, A_START + 60 + 3)          # exactly at the right edge junction: q_hi behind it, the inserted bases inside
    assert one(ins, 159, 1, 2) == (A_START + 57, A_START + 62 + 3)          # inside
    assert one(ins, 163, 1, 2) == (A_START + 64, A_START + 69)              # one base further right: the insertion is outside
    assert one(ins, 160, 0, 0) == (A_START + 60, A_START + 63)              # |ref| 0, flank 0: the inserted bases alone
    assert one("200=", 160, 0, 0) is None                                   # ... and nothing where there is no insertion
    assert one(ins, 160, 0, 2) == (A_START + 58, A_START + 65)              # the default flank puts the junction strictly inside
    # "50= 30D 120=": the deletion covers backbone [150, 180); query offset 57 on both sides of it
    dele = "50= 30D 120="
    assert one(dele, 160, 5, 2) is None                                     # [158, 167) lies under the one D: none
    assert one(dele, 150, 1, 0) is None and one(dele, 179, 1, 0) is None
    assert one(dele, 148, 5, 0) == (A_START + 48, A_START + 50)             # a D crossing the right edge: the window ends where the deletion begins
    assert one(dele, 178, 5, 0) == (A_START + 50, A_START + 53)             # a D crossing the left edge
    assert one(dele, 149, 1, 2) == (A_START + 47, A_START + 50) and one(dele, 181, 1, 2) == (A_START + 50, A_START + 54)
    assert one(dele, 145, 40, 0) == (A_START + 45, A_START + 55)            # the D inside the interval


def test_bad_arguments(pkg):
    db, ffi = pkg.database, pkg.ffi
    ops = ref.ops_of("50= 2I 50=")
    a = aln_of(ffi, ops)
    a[0]["b_end"] += 1                                                      # the ops do not consume the span
    with pytest.raises(pkg.StarphaseError):
        db.cyp_variant_windows(a, ops, [150], [1], 2)
    assert db.cyp_variant_windows(aln_of(ffi, ops), [], [150], [1], 2) == [None]          # no alignment: no window
    assert db.cyp_variant_windows(aln_of(ffi, ops), ops, [], [], 2) == []

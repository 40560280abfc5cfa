"""The alignment contract of DESIGN.md 3.1 / 3.2 as a plain statement (tests/align_contract_ref.py: a dictionary and a row-by-row DP) against oracle/align.c (a
wavefront algorithm, like the kernels) on the designed cases of tests/align_contract_cases.py.  The plain statement decides: the oracle's (ok, nm, a_end, b_end)
must equal it on 64 diagonals, on 256 and under sp_align_batch's rule, its anchors must equal it, and its events must spell an alignment of that cost."""
import numpy as np
import pytest

import align_contract_cases as cases
import align_contract_ref as ref

CELL_FAMILIES = sorted(cases.cell_families())
ANCHOR_FAMILIES = sorted(cases.anchor_families())


# ------------------------------------------------------------------------------------------------ the reference against simpler statements of itself
def test_reference_cell_equals_full_matrix():
    """lengths up to 12: 64 diagonals around a diagonal in -19 .. 20 hold the whole rectangle, so the banded row DP is the full ends-free matrix"""
    rng = np.random.default_rng(4001)
    for t in range(1500):
        la, lb = int(rng.integers(1, 13)), int(rng.integers(1, 13))
        letters = "ACGTN" if t % 3 else "AC"
        a = "".join(letters[x] for x in rng.integers(0, len(letters), la))
        b = "".join(letters[x] for x in rng.integers(0, len(letters), lb))
        if t % 4 == 0 and la > 3:
            b = a[1:] + b[:2]
        diag = int(rng.integers(-19, 21))
        got, want = ref.cell(a, b, diag, 64), ref.full_matrix(a, b)
        assert got[0][0] == want[0] and got[1] == want[1], (a, b, diag, got, want)
        assert (got[0][1], got[0][2]) in want[1]
        wide = ref.cell(a, b, diag, 256)
        assert wide[0][0] == want[0] and wide[1] == want[1], (a, b, diag, wide, want)


def test_reference_anchor_equals_bruteforce():
    rng = np.random.default_rng(4002)
    for t in range(150):
        unit = cases.rseq(rng, int(rng.integers(16, 30)))
        a = "".join(cases.rseq(rng, int(rng.integers(0, 40))) + unit for _ in range(int(rng.integers(1, 7))))
        b = cases.rseq(rng, int(rng.integers(0, 60))) + unit + cases.rseq(rng, int(rng.integers(0, 30))) + a[:int(rng.integers(0, 50))]
        if t % 5 == 0:
            b = cases.put(b, int(rng.integers(0, len(b))), "N")
        if t % 7 == 0:
            a = cases.put(a, int(rng.integers(0, len(a))), "N")
        assert ref.anchor_topk(a, b, 4) == ref.anchor_bruteforce(a, b, 4), (a, b)
    for c in cases.anchor_families()["short"] + cases.anchor_families()["occurrences"][:2] + cases.anchor_families()["peaks"][:12]:
        assert ref.anchor_topk(c.a, c.b, 4) == ref.anchor_bruteforce(c.a, c.b, 4), c.name


def test_replay_rejects_what_is_not_an_alignment():
    a, b = "ACGTACGTAC", "ACGAACGTAC"
    ref.replay(a, b, 64, 0, (1, 0, 10, 0, 10), [(ref.EV_X << 30) | 3])
    for aln, ev in (((1, 0, 10, 0, 10), [(ref.EV_X << 30) | 4]),          # X on a match, and a mismatch walked over as a match
                    ((0, 0, 10, 0, 10), []),                                # the mismatch is not paid
                    ((1, 0, 9, 0, 9), [(ref.EV_X << 30) | 3]),              # ends inside the rectangle
                    ((1, 1, 10, 1, 10), [(ref.EV_X << 30) | 3]),            # starts inside the rectangle
                    ((2, 0, 10, 0, 10), [(ref.EV_X << 30) | 3])):           # nm is not the number of events
        with pytest.raises(AssertionError):
            ref.replay(a, b, 64, 0, aln, ev)
    with pytest.raises(AssertionError):                                     # a diagonal outside the band
        ref.replay(a, b, 64, 40, (1, 0, 10, 0, 10), [(ref.EV_X << 30) | 3])


# ------------------------------------------------------------------------------------------------ what the families are meant to reach
def test_case_families_reach_what_they_aim_at():
    fams = cases.cell_families()
    by_name = {c.name: c for f in fams.values() for c in f}
    assert sum(c.name.startswith("fuzz_") for c in fams["fuzz"]) == 300
    # every rule of the end order is needed by some pair
    for kind in ("path", "central", "lowest"):
        ties = [c for c in fams["end_ties"] if c.name.startswith(f"tie_{kind}_")]
        assert len(ties) == 8 and all(cases.end_tie_kind(c.a, c.b, c.diag) == kind for c in ties), kind
    assert all(cases.end_tie_kind(c.a, c.b, c.diag) for c in fams["end_ties"][:4])
    # the second try: narrow found with more than 32 edits both times; the wide run strictly cheaper once, not cheaper once
    c = by_name["retry2_wide_strictly_cheaper"]
    n64, n256 = cases.ref_cell(c.a, c.b, c.diag, 64)[0][0], cases.ref_cell(c.a, c.b, c.diag, 256)[0][0]
    assert 32 < n256 < n64 <= c.max_ed and cases.ref_align(c)[3] == 256
    c = by_name["retry2_wide_not_cheaper"]
    n64, n256 = cases.ref_cell(c.a, c.b, c.diag, 64)[0][0], cases.ref_cell(c.a, c.b, c.diag, 256)[0][0]
    assert 32 < n256 == n64 <= c.max_ed and cases.ref_align(c)[3] == 64
    # the library's cap
    c = by_name["cap_511_edits_exactly"]
    assert cases.ref_cell(c.a, c.b, c.diag, 256)[0][0] == 511 and cases.ref_align(c)[0] == 511
    c = by_name["cap_512_edits_lost"]
    assert cases.ref_cell(c.a, c.b, c.diag, 256)[0][0] == 512 and cases.ref_align(c) is None
    # the drifts: found up to the last lane of the wide band, lost beyond it
    for c in fams["band_edges"]:
        if c.name.startswith("drift_"):
            drift = int(c.name.split("_")[1])
            r = cases.ref_align(c)
            assert (r is None) == (drift > 127 or drift < -128), c.name
            if r is not None:
                assert r[0] == abs(drift) and r[3] == (64 if abs(drift) <= 32 and -32 <= drift <= 31 else 256), (c.name, r)
    # a 16-mer that occurs four times votes four times, one that occurs five times does not vote
    occ = {c.name: cases.ref_anchor(c.a, c.b, 4) for c in cases.anchor_families()["occurrences"]}
    assert [v for _, v in occ["kmer_occurs_4_times_alone"]] == [1, 1, 1, 1] and [v for _, v in occ["kmer_occurs_5_times_alone"]] == [0, 0, 0, 0]
    assert [v for _, v in occ["kmer_occurs_4_times_beside_unique"]] == [9, 1, 1, 1] and [v for _, v in occ["kmer_occurs_5_times_beside_unique"]] == [9, 0, 0, 0]
    # an N kills exactly the 16 windows over it (one at the first and the last base)
    nw = {c.name: cases.ref_anchor(c.a, c.b, 1)[0][1] for c in cases.anchor_families()["n_windows"]}
    assert nw["n_in_looked_up_at100"] == nw["n_in_indexed_at100"] == 185 - 16 and nw["n_in_looked_up_at0"] == nw["n_in_indexed_at199"] == 184
    assert nw["n_every_16th_no_window"] == 0
    # the anchor table of the last family does not fit in LDS beside the bins (160 KB - 64 bytes of LDS, 2 bytes per bin, 8 per table entry)
    big = cases.anchor_families()["global_table"]
    m, n = max(len(c.a) for c in big), max(len(c.b) for c in big)
    assert (m + n + 2) // 2 * 4 + 8 * m > 160 * 1024 - 64


def test_only_the_named_cases_are_lost():
    """under sp_align_batch's rule the reference finds every pair but: a band that misses the rectangle, a drift no band holds, a cap below the cost.  In the fuzz
    it finds at least 80 % of the pairs on 64 diagonals alone."""
    for fam, cs in cases.cell_families().items():
        for c in cs:
            if not c.may_lose:
                assert cases.ref_align(c) is not None, c.name
    marked = {c.name for cs in cases.cell_families().values() for c in cs if c.may_lose and not c.name.startswith("fuzz_")}
    assert all(n.startswith(("band_misses_", "drift_+128", "drift_+129", "drift_-129", "cap_below_cost_", "cap_zero_", "cap_512_")) for n in marked), marked
    fuzz = cases.cell_families()["fuzz"]
    found = 0
    for c in fuzz:
        r = cases.ref_cell(c.a, c.b, c.diag, 64)
        found += r is not None and r[0][0] <= c.max_ed
    print(f"fuzz: the reference finds {found} of {len(fuzz)} pairs on 64 diagonals")
    assert found >= 0.8 * len(fuzz)


# ------------------------------------------------------------------------------------------------ the oracle against the reference
def _row(al):
    return (al.ok, al.nm, al.a_end, al.b_end)


def _replay(c, band, al, ev):
    try:
        ref.replay(c.a, c.b, band, c.diag, (al.nm, al.a_start, al.a_end, al.b_start, al.b_end), ev)
    except AssertionError as e:
        raise AssertionError((c.name, "replay", band) + e.args) from None


@pytest.mark.parametrize("family", CELL_FAMILIES)
def test_oracle_cell_against_reference(oracle, family):
    lost = 0
    for c in cases.cell_families()[family]:
        A, B = oracle.encode(c.a), oracle.encode(c.b)
        for band in (64, 256):
            want = cases.ref_cell(c.a, c.b, c.diag, band)
            for cap in sorted({ref.MAX_ED, c.max_ed}):
                al, ev = oracle.wfa(A, B, c.diag, cap, band=band)
                exp = (1,) + want[0] if want is not None and want[0][0] <= cap else (0, 0, 0, 0)
                assert _row(al) == exp, (c.name, band, cap, _row(al), exp)
                if al.ok:
                    _replay(c, band, al, ev)
        want = cases.ref_align(c)
        al, ev = oracle.wfa(A, B, c.diag, c.max_ed, retry=2)
        assert _row(al) == ((1,) + want[:3] if want else (0, 0, 0, 0)), (c.name, "retry2", _row(al), want)
        if want:
            _replay(c, want[3], al, ev)
        lost += want is None
    print(f"{family}: {len(cases.cell_families()[family])} cases, {lost} lost")


@pytest.mark.parametrize("family", ANCHOR_FAMILIES)
def test_oracle_anchor_against_reference(oracle, family):
    for c in cases.anchor_families()[family]:
        want = cases.ref_anchor(c.a, c.b, 4)
        assert tuple(oracle.anchor_topk(c.a, c.b, 4)) == want, (c.name, want)
        assert oracle.anchor(c.a, c.b) == want[0], (c.name, want)
        assert tuple(oracle.anchor_topk(c.a, c.b, 1)) == want[:1], c.name


@pytest.mark.parametrize("family", CELL_FAMILIES)
def test_oracle_anchor_on_the_cell_cases(oracle, family):
    """the pairs of the cell families as anchor cases (B indexed, as the cell's callers do it)"""
    for c in cases.cell_families()[family]:
        want = cases.ref_anchor(c.b, c.a, 4)
        assert tuple(oracle.anchor_topk(c.b, c.a, 4)) == want, (c.name, want)

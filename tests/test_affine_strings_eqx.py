"""sp_affine_cigar_strings_eqx (host only): sp_affine_cigar_strings with '=' and 'X' runs kept apart, as minimap2 writes a CIGAR under --eqx -- score_read maps with
that flag (src/hla/caller.rs:1395), so the cigar of hla_debug.json's per-allele mappings carries them.  MD and match_len are the existing function's."""
import re

import numpy as np
import pytest

from test_affine_strings import OP, random_columns


@pytest.fixture(scope="module")
def D(pkg):
    return pkg.database


def expected_eqx(cols):
    """the restatement: runs of equal column kinds, nothing merged"""
    out, last, run = "", None, 0
    for c, _ in cols:
        if c == last:
            run += 1
        else:
            if run:
                out += f"{run}{last}"
            last, run = c, 1
    if run:
        out += f"{run}{last}"
    return out


def test_eqx_strings_of_random_op_lists(D):
    rng = np.random.default_rng(21)
    x_next_to_eq = 0
    for _ in range(200):
        target, query, aln, cols, ops = random_columns(rng)
        cigar, md, match_len = D.affine_cigar_strings_eqx(aln, ops, target)
        merged, md0, match_len0 = D.affine_cigar_strings(aln, ops, target)
        assert cigar == expected_eqx(cols)
        assert (md, match_len) == (md0, match_len0)                      # MD and match_len do not depend on the spelling of the CIGAR
        runs = [(int(n), op) for n, op in re.findall(r"(\d+)([=XID])", cigar)]
        assert "".join(f"{n}{op}" for n, op in runs) == cigar
        assert [(n, OP[op]) for n, op in runs] == [(int(w) >> 4, int(w) & 15) for w in ops]      # the ops, run for run
        assert all(a[1] != b[1] for a, b in zip(runs, runs[1:]))
        assert sum(n for n, op in runs if op == "=") == match_len
        assert sum(n for n, op in runs if op in "XID") == aln["nm"]
        # merging '=' and 'X' gives the existing function's string
        back, last = [], None
        for n, op in runs:
            op = "M" if op in "=X" else op
            if back and back[-1][1] == op:
                back[-1] = (back[-1][0] + n, op)
            else:
                back.append((n, op))
        assert "".join(f"{n}{op}" for n, op in back) == merged
        x_next_to_eq += bool(re.search(r"=\d+X|X\d+=", cigar))
    assert x_next_to_eq >= 150


def test_eqx_edge_cases_and_capacity(D, pkg):
    target = "ACGTACGTAC"
    full = dict(score=10, nm=0, a_start=0, a_end=10, b_start=0, b_end=10)
    assert D.affine_cigar_strings_eqx(full, [10 << 4 | 7], target) == ("10=", "10", 10)
    ops = [1 << 4 | 8, 2 << 4 | 2, 1 << 4 | 8, 1 << 4 | 1, 6 << 4 | 7]
    assert D.affine_cigar_strings_eqx(dict(full, nm=5, a_end=9), ops, target) == ("1X2D1X1I6=", "0A0^CG0T6", 6)
    assert D.affine_cigar_strings_eqx(dict(full, nm=2, a_end=10), [3 << 4 | 7, 2 << 4 | 8, 5 << 4 | 7], target) == ("3=2X5=", "3T0A5", 8)
    assert D.affine_cigar_strings_eqx(dict(full, nm=0, a_end=0, b_end=0, score=0), [], target) == ("", "0", 0)
    for bad in ([9 << 4 | 7], [11 << 4 | 7], [10 << 4 | 0], [10 << 4 | 7, 1 << 4 | 1], [0 << 4 | 7, 10 << 4 | 7]):
        with pytest.raises(pkg.StarphaseError):
            D.affine_cigar_strings_eqx(full, bad, target)
    with pytest.raises(pkg.StarphaseError) as e:
        D.affine_cigar_strings_eqx(dict(full, nm=5, a_end=9), ops, target, cigar_cap=4)
    assert e.value.code == 6
    with pytest.raises(pkg.StarphaseError) as e:
        D.affine_cigar_strings_eqx(dict(full, nm=5, a_end=9), ops, target, md_cap=4)
    assert e.value.code == 6

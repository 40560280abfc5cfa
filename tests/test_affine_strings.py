"""sp_affine_cigar_strings (host only): the CIGAR string, MD tag and match_len DetailedMappingStats::from_mapping copies from minimap2, made from the ops of
sp_affine_align_batch / sp_hla_realign_cigars ('=' and 'X' merge into M; MD prints the target base of an 'X' column and ^bases of a deletion) -- the formatting
rules of sp_aln_strings, stated by tests/test_debug_files.py::expected_strings -- and a read_debug.json made from such strings through sp_hla_debug_*."""
import json
import re

import numpy as np
import pytest

from test_debug_files import expected_strings

OP = {"=": 7, "X": 8, "I": 1, "D": 2}


@pytest.fixture(scope="module")
def D(pkg):
    return pkg.database


def random_columns(rng, n=300):
    """target, query, spans and the alignment column by column; gaps may open and close the span, '=' and 'X' runs meet, deletions are followed by mismatches"""
    target = "".join(rng.choice(list("ACGT"), n))
    b_start, b_end = int(rng.integers(0, 20)), n - int(rng.integers(0, 20))
    a_start = int(rng.integers(0, 10))
    cols, query = [], list(rng.choice(list("ACGT"), a_start))
    j, mode = b_start, int(rng.integers(0, 4))
    if mode == 1:                                            # a leading insertion / deletion inside the span
        k = int(rng.integers(1, 4)); cols += [("I", None)] * k; query += list(rng.choice(list("ACGT"), k))
    elif mode == 2:
        k = int(rng.integers(1, 4)); cols += [("D", target[j + x]) for x in range(k)]; j += k
    while j < b_end:
        u = rng.random()
        after_del = bool(cols) and cols[-1][0] == "D"
        if u < 0.04 or (after_del and u < 0.5):               # (half of the deletions are followed by a mismatch: MD "^AC0T")
            cols.append(("X", target[j])); query.append(rng.choice([c for c in "ACGT" if c != target[j]])); j += 1
        elif u < 0.07:
            k = min(int(rng.integers(1, 30)), b_end - j); cols += [("D", target[j + x]) for x in range(k)]; j += k
        elif u < 0.10:
            k = int(rng.integers(1, 30)); cols += [("I", None)] * k; query += list(rng.choice(list("ACGT"), k))
        else:
            cols.append(("=", target[j])); query.append(target[j]); j += 1
    if mode == 3:                                            # a trailing insertion inside the span
        cols += [("I", None)] * 2; query += ["A", "C"]
    a_end = len(query)
    query += list(rng.choice(list("ACGT"), int(rng.integers(0, 10))))
    ops = []
    for c, _ in cols:
        if ops and ops[-1][1] == OP[c]:
            ops[-1] = (ops[-1][0] + 1, OP[c])
        else:
            ops.append((1, OP[c]))
    nm = sum(1 for c, _ in cols if c != "=")
    aln = dict(score=1, nm=nm, a_start=a_start, a_end=a_end, b_start=b_start, b_end=b_end)
    return target, "".join(query), aln, cols, np.array([n << 4 | op for n, op in ops], np.uint32)


def test_strings_of_random_op_lists(D):
    rng = np.random.default_rng(9)
    seen_del_then_x = 0
    for _ in range(300):
        target, query, aln, cols, ops = random_columns(rng)
        cigar, md, match_len = D.affine_cigar_strings(aln, ops, target)
        assert (cigar, md, match_len) == expected_strings(cols)
        seen_del_then_x += bool(re.search(r"\^[ACGT]+0[ACGT]", md))
        # round trip: the ops rebuilt from (CIGAR string, MD) consume the spans and give nm
        cg = [(int(n), op) for n, op in re.findall(r"(\d+)([MID])", cigar)]
        assert "".join(f"{n}{op}" for n, op in cg) == cigar
        assert sum(n for n, op in cg if op in "MD") == aln["b_end"] - aln["b_start"] and sum(n for n, op in cg if op in "MI") == aln["a_end"] - aln["a_start"]
        mismatches = deleted = matched = 0
        rebuilt = []
        for num, dele, mis in re.findall(r"(\d+)|\^([ACGT]+)|([ACGT])", md):
            if num:
                matched += int(num)
            elif dele:
                deleted += len(dele); rebuilt.append(dele)
            else:
                mismatches += 1
        assert matched == match_len and matched + mismatches == sum(n for n, op in cg if op == "M") and deleted == sum(n for n, op in cg if op == "D")
        assert mismatches + deleted + sum(n for n, op in cg if op == "I") == aln["nm"]
        aligned_query, qpos = [], aln["a_start"]              # MD rebuilds the target from the query bases of the M columns
        for n, op in cg:
            if op == "M":
                aligned_query += list(query[qpos:qpos + n])
            if op in "MI":
                qpos += n
        out, k = [], 0
        for num, dele, mis in re.findall(r"(\d+)|\^([ACGT]+)|([ACGT])", md):
            if num:
                out += aligned_query[k:k + int(num)]; k += int(num)
            elif dele:
                out += list(dele)
            else:
                out.append(mis); k += 1
        assert "".join(out) == target[aln["b_start"]:aln["b_end"]]
    assert seen_del_then_x >= 20


def test_edge_cases_and_capacity(D, pkg):
    target = "ACGTACGTAC"
    full = dict(score=10, nm=0, a_start=0, a_end=10, b_start=0, b_end=10)
    assert D.affine_cigar_strings(full, [10 << 4 | 7], target) == ("10M", "10", 10)
    ops = [1 << 4 | 8, 2 << 4 | 2, 1 << 4 | 8, 1 << 4 | 1, 6 << 4 | 7]                          # X, DD, X, I, six matches: the case of test_debug_files.py
    assert D.affine_cigar_strings(dict(full, nm=5, a_end=9), ops, target) == ("1M2D1M1I6M", "0A0^CG0T6", 6)
    assert D.affine_cigar_strings(dict(full, nm=0, a_end=0, b_end=0, score=0), [], target) == ("", "0", 0)      # score 0: no ops, empty spans
    for bad in ([9 << 4 | 7], [11 << 4 | 7], [10 << 4 | 0], [10 << 4 | 7, 1 << 4 | 1], [0 << 4 | 7, 10 << 4 | 7]):
        with pytest.raises(pkg.StarphaseError):              # ops that do not consume exactly the spans, an op of another kind, an empty op
            D.affine_cigar_strings(full, bad, target)
    # buffers that are too small: SP_ERR_CAPACITY and the text cut short, as sp_aln_strings does
    with pytest.raises(pkg.StarphaseError) as e:
        D.affine_cigar_strings(dict(full, nm=5, a_end=9), ops, target, cigar_cap=4)
    assert e.value.code == 6
    with pytest.raises(pkg.StarphaseError) as e:
        D.affine_cigar_strings(dict(full, nm=5, a_end=9), ops, target, md_cap=4)
    assert e.value.code == 6


def test_read_debug_json_layout(D):
    """read_debug.json is an HlaDebug object: per gene and QNAME the accepted allele and its DNA mapping, no cDNA mapping, no dual statistics"""
    rng = np.random.default_rng(10)
    dbg = D.HlaDebug()
    expected = {}
    for gene, qname, allele, star in (("HLA-A", "m1/12/ccs", "HLA:HLA00001", "01:01:01:01"), ("HLA-A", "m1/7/ccs", "HLA:HLA00005", "02:01:01:01"), ("HLA-B", "m1/3/ccs", "HLA:HLA00132", "07:02:01:01")):
        target, query, aln, cols, ops = random_columns(rng)
        dm = D.affine_detailed_mapping(aln, ops, target, len(query))
        cigar, md, match_len = expected_strings(cols)
        assert dm == dict(query_len=len(query), target_len=len(target), match_len=match_len, nm=aln["nm"], query_unmapped=len(query) - (aln["a_end"] - aln["a_start"]),
                          target_unmapped=len(target) - (aln["b_end"] - aln["b_start"]), cigar=cigar, md=md)
        dbg.add_read(gene, qname, allele, star)
        dbg.add_mapping(gene, qname, allele, cdna=None, dna=dm)
        expected.setdefault(gene, {})[qname] = {"best_match_id": allele, "best_match_star": star, "mapping_stats": {allele: {"cdna_mapping": None, "dna_mapping": dm}}}
    got = json.loads(dbg.json())
    assert got == {"read_mapping_stats": expected, "dual_passing_stats": None}
    assert list(got["read_mapping_stats"]["HLA-A"]) == ["m1/12/ccs", "m1/7/ccs"]               # BTreeMap order

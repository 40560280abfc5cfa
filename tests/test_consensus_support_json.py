"""consensus_support.json and the summary rule behind it, on hand-made counts (host only: no device is touched)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import pileup_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def table(ffi, rows):
    """rows of (depth, eq, (xa, xc, xg, xt), del, ins)"""
    cols = np.zeros(len(rows), ffi.PILEUP_DTYPE)
    for j, (depth, eq, x, dl, ins) in enumerate(rows):
        cols[j] = (depth, eq, x, dl, ins)
    return cols


def test_summary_rule_and_lower_median(pkg):
    ffi = pkg.ffi
    # depths 4 8 7 1: even length, the lower median of (1, 4, 7, 8) is 4; column 1 has eq exactly half (contested), column 3 an insertion majority
    even = table(ffi, [(4, 3, (0, 1, 0, 0), 0, 2), (8, 4, (0, 0, 4, 0), 0, 0), (7, 7, (0, 0, 0, 0), 0, 3), (1, 1, (0, 0, 0, 0), 0, 1)])
    got = ffi.support_summarize(even, n_members=11, n_aligned=9)
    assert got == dict(n_members=11, n_aligned=9, n_unaligned=2, length=4, min_depth=1, median_depth=4, n_contested=2)
    assert list(ffi.support_contested(even)) == [1, 3]
    odd = table(ffi, [(5, 5, (0, 0, 0, 0), 0, 0), (2, 2, (0, 0, 0, 0), 0, 1), (8, 5, (1, 1, 1, 0), 0, 4)])
    assert ffi.support_summarize(odd, 8, 8) == dict(n_members=8, n_aligned=8, n_unaligned=0, length=3, min_depth=2, median_depth=5, n_contested=0)
    for tab, members, aligned in ((even, 11, 9), (odd, 8, 8)):
        assert ffi.support_summarize(tab, members, aligned) == pileup_ref.summary(pileup_ref.as_table(tab), members, aligned)
        assert list(ffi.support_contested(tab)) == pileup_ref.contested(pileup_ref.as_table(tab))
    # a column nobody spans is not contested; one with an insertion behind it and no depth would be (2 * ins > depth), which no pileup produces
    zero = table(ffi, [(0, 0, (0, 0, 0, 0), 0, 0), (3, 1, (0, 0, 0, 0), 2, 0), (3, 2, (1, 0, 0, 0), 0, 0)])
    assert list(ffi.support_contested(zero)) == [1]
    assert ffi.support_summarize(zero, 3, 3)["min_depth"] == 0
    assert ffi.support_summarize(table(ffi, []), 0, 0) == dict(n_members=0, n_aligned=0, n_unaligned=0, length=0, min_depth=0, median_depth=0, n_contested=0)
    with pytest.raises(pkg.StarphaseError):
        ffi.support_summarize(odd, 2, 3)                     # more aligned members than members


def test_consensus_support_json_layout(pkg):
    ffi = pkg.ffi
    a1 = table(ffi, [(10, 10, (0, 0, 0, 0), 0, 0), (10, 4, (0, 6, 0, 0), 0, 0), (9, 8, (0, 0, 0, 0), 1, 5), (0, 0, (0, 0, 0, 0), 0, 0)])
    a2 = table(ffi, [(6, 6, (0, 0, 0, 0), 0, 0), (6, 6, (0, 0, 0, 0), 0, 0), (5, 5, (0, 0, 0, 0), 0, 0)])
    b1 = table(ffi, [(3, 1, (1, 0, 0, 1), 0, 0)])
    sm = lambda tab, m, a: ffi.support_summarize(tab, m, a)
    entries = [("HLA-B", [("HLA-B*07:02:01:01", "G", b1, sm(b1, 3, 3)), None]),
               ("HLA-DRB5", [None, None]),                                             # no call: omitted
               ("HLA-A", [("HLA-A*01:01:01:01", "ACGT", a1, sm(a1, 12, 10)), (None, "TTA", a2, sm(a2, 6, 6))])]
    text = ffi.consensus_support_json(entries)
    col = lambda pos, depth, eq, x, dl, ins, base: {"pos": pos, "depth": depth, "eq": eq, "x": list(x), "del": dl, "ins": ins, "consensus_base": base}
    expected = {
        "HLA-A": {
            "consensus1": {"n_members": 12, "n_aligned": 10, "n_unaligned": 2, "length": 4, "min_depth": 0, "median_depth": 9, "n_contested": 2,
                           "typed_allele": "HLA-A*01:01:01:01", "contested": [col(1, 10, 4, (0, 6, 0, 0), 0, 0, "C"), col(2, 9, 8, (0, 0, 0, 0), 1, 5, "G")]},
            "consensus2": {"n_members": 6, "n_aligned": 6, "n_unaligned": 0, "length": 3, "min_depth": 5, "median_depth": 6, "n_contested": 0,
                           "typed_allele": None, "contested": []}},
        "HLA-B": {
            "consensus1": {"n_members": 3, "n_aligned": 3, "n_unaligned": 0, "length": 1, "min_depth": 3, "median_depth": 3, "n_contested": 1,
                           "typed_allele": "HLA-B*07:02:01:01", "contested": [col(0, 3, 1, (1, 0, 0, 1), 0, 0, "G")]}}}
    assert text == json.dumps(expected, indent=2)                # gene order, field order, omitted genes, the empty list, indentation
    assert ffi.consensus_support_json([]) == "{}"
    # a consensus whose length is not its summary's, and a gene given twice, are refused
    with pytest.raises(pkg.StarphaseError):
        ffi.consensus_support_json([("HLA-A", [("x", "ACG", a1, sm(a1, 1, 1)), None])])
    with pytest.raises(pkg.StarphaseError):
        ffi.consensus_support_json([("HLA-B", [("x", "G", b1, sm(b1, 3, 3)), None]), ("HLA-B", [("x", "G", b1, sm(b1, 3, 3)), None])])
    small = C.create_string_buffer(8)
    arr = (ffi.sp_support_entry * 1)()
    arr[0].gene = b"HLA-A"
    need = C.c_uint64(0)
    assert ffi.lib().sp_consensus_support_json(arr, 1, small, 8, C.byref(need)) == ffi.SP_OK and small.value == b"{}" and need.value == 3


def test_new_symbols_in_header_rust_block_and_binding(pkg):
    import inspect
    header = open(os.path.join(ROOT, "include", "starphase_hip.h")).read()
    rs = open(os.path.join(ROOT, "include", "starphase_hip.rs")).read()
    src = inspect.getsource(pkg.ffi)
    L = pkg.ffi.lib()
    for name in ("sp_pileup_batch", "sp_support_summarize", "sp_support_contested", "sp_hla_consensus_support", "sp_hla_consensus_support_cohort",
                 "sp_consensus_support_json"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert "pub fn %s(" % name in rs, name
        assert '"%s"' % name in src, name
        assert hasattr(L, name), name
    assert L.sp_struct_size(b"sp_pileup_col") == pkg.ffi.PILEUP_DTYPE.itemsize == 32
    assert L.sp_struct_size(b"sp_support_summary") == C.sizeof(pkg.ffi.sp_support_summary) == pkg.ffi.SUPPORT_DTYPE.itemsize == 32
    assert L.sp_struct_size(b"sp_support_entry") == C.sizeof(pkg.ffi.sp_support_entry)
    # the tile geometry the GPU tests straddle is the header's
    assert int(re.search(r"#define SP_PILEUP_TILE\s+(\d+)", header).group(1)) == pkg.ffi.SP_PILEUP_TILE
    assert int(re.search(r"#define SP_PILEUP_WAVES\s+(\d+)", header).group(1)) == pkg.ffi.SP_PILEUP_WAVES

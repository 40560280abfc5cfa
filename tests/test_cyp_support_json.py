"""cyp2d6_consensus_support.json (sp_cyp_support_json) on hand-made counts: host only, no device is touched."""
import json

import numpy as np


def table(ffi, rows):
    """rows of (depth, eq, (xa, xc, xg, xt), del, ins)"""
    cols = np.zeros(len(rows), ffi.PILEUP_DTYPE)
    for j, (depth, eq, x, dl, ins) in enumerate(rows):
        cols[j] = (depth, eq, x, dl, ins)
    return cols


def make_call(ffi, regions, status=0):
    """regions: [(cons_type, cons_subtype or None)]"""
    call = ffi.sp_cyp_call()
    call.status = status
    call.n_consensus = len(regions)
    for h, (t, sub) in enumerate(regions):
        call.cons_type[h] = t
        call.cons_subtype[h].value = (sub or "").encode()
    return call


# SP_CYP_* region types (include/starphase_hip.h)
REP6, CYP2D6, LINK, CYP2D7, HYBRID = 1, 2, 3, 6, 8


def example(pkg):
    ffi = pkg.ffi
    d6 = table(ffi, [(10, 10, (0, 0, 0, 0), 0, 0), (10, 4, (0, 6, 0, 0), 0, 0), (9, 8, (0, 0, 0, 0), 1, 5), (0, 0, (0, 0, 0, 0), 0, 0)])
    d7 = table(ffi, [(6, 6, (0, 0, 0, 0), 0, 0), (6, 6, (0, 0, 0, 0), 0, 0), (5, 5, (0, 0, 0, 0), 0, 0)])
    hyb = table(ffi, [(3, 1, (1, 0, 0, 1), 0, 0)])
    call = make_call(ffi, [(CYP2D6, "4.001"), (CYP2D7, None), (HYBRID, 'CYP2D6::CYP2D7::exon9 "q"\\'), (LINK, None)])
    cons = ["ACGT", "TTA", "G", ""]
    cols = [d6, d7, hyb, table(ffi, [])]
    sums = [ffi.support_summarize(d6, 12, 10), ffi.support_summarize(d7, 6, 6), ffi.support_summarize(hyb, 3, 3), ffi.support_summarize(cols[3], 0, 0)]
    return call, cons, cols, sums


def test_layout_key_order_and_escaping(pkg):
    call, cons, cols, sums = example(pkg)
    text = pkg.database.cyp_support_json(call, cons, cols, sums)
    col = lambda pos, depth, eq, x, dl, ins, base: {"pos": pos, "depth": depth, "eq": eq, "x": list(x), "del": dl, "ins": ins, "consensus_base": base}
    label = 'CYP2D6::CYP2D7::exon9 "q"\\'
    expected = {
        "0_CYP2D6*4.001": {"n_members": 12, "n_aligned": 10, "n_unaligned": 2, "length": 4, "min_depth": 0, "median_depth": 9, "n_contested": 2, "region_type": "CYP2D6*4.001",
                           "contested": [col(1, 10, 4, (0, 6, 0, 0), 0, 0, "C"), col(2, 9, 8, (0, 0, 0, 0), 1, 5, "G")]},
        "1_CYP2D7": {"n_members": 6, "n_aligned": 6, "n_unaligned": 0, "length": 3, "min_depth": 5, "median_depth": 6, "n_contested": 0, "region_type": "CYP2D7", "contested": []},
        "2_" + label: {"n_members": 3, "n_aligned": 3, "n_unaligned": 0, "length": 1, "min_depth": 3, "median_depth": 3, "n_contested": 1, "region_type": label,
                       "contested": [col(0, 3, 1, (1, 0, 0, 1), 0, 0, "G")]},
        "3_link_region": {"n_members": 0, "n_aligned": 0, "n_unaligned": 0, "length": 0, "min_depth": 0, "median_depth": 0, "n_contested": 0, "region_type": "link_region",
                          "contested": []}}
    got = json.loads(text)
    assert got == expected
    assert list(got) == list(expected)                                            # consensus order, not name order
    for entry in got.values():
        assert list(entry) == ["n_members", "n_aligned", "n_unaligned", "length", "min_depth", "median_depth", "n_contested", "region_type", "contested"]
    assert list(got["0_CYP2D6*4.001"]["contested"][0]) == ["pos", "depth", "eq", "x", "del", "ins", "consensus_base"]
    assert text == json.dumps(expected, indent=2)                                 # two-space indent, an empty list as []
    assert '\\"q\\"\\\\' in text                                                   # the label's quote and backslash are escaped


def test_a_failed_call_has_no_entries(pkg):
    call, cons, cols, sums = example(pkg)
    call.status = 16
    assert pkg.database.cyp_support_json(call, cons, cols, sums) == "{}"
    assert pkg.database.cyp_support_json(make_call(pkg.ffi, []), [], [], []) == "{}"


def test_cap_and_needed(pkg):
    ffi = pkg.ffi
    call, cons, cols, sums = example(pkg)
    text = pkg.database.cyp_support_json(call, cons, cols, sums)
    need = len(text.encode()) + 1
    rc, out, needed = pkg.database.cyp_support_json(call, cons, cols, sums, cap=0)
    assert rc == ffi.SP_ERR_CAPACITY and needed == need
    rc, out, needed = pkg.database.cyp_support_json(call, cons, cols, sums, cap=need - 1)
    assert rc == ffi.SP_ERR_CAPACITY and needed == need and out == ""
    rc, out, needed = pkg.database.cyp_support_json(call, cons, cols, sums, cap=need)
    assert rc == ffi.SP_OK and needed == need and out == text


def test_a_table_that_does_not_fit_its_summary_is_refused(pkg):
    ffi = pkg.ffi
    call, cons, cols, sums = example(pkg)
    sums[1] = dict(sums[1], length=2)                                             # three columns, a summary of two
    rc, out, needed = pkg.database.cyp_support_json(call, cons, cols, sums, cap=4096)
    assert rc == ffi.SP_ERR_INVALID_ARG

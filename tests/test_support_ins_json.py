"""sp_consensus_support_json_ins and sp_cyp_support_json_ins on hand-made counts and records, against a json.dumps(indent=2) statement: host only, no device is touched."""
import json

import numpy as np

import pileup_ins_ref as ref
from test_cyp_support_json import CYP2D6, CYP2D7, make_call, table


def records(ffi, rows):
    """rows of (col, string, count, first_pair, n_other); a string of '' is a column's len-0 record"""
    out = np.zeros(len(rows), ffi.INS_DTYPE)
    for k, (col, s, count, first, other) in enumerate(rows):
        n, p0, p1, h = ref.key_of(s) if s else (0, 0, 0, 0)
        out[k] = (col, n, count, p0, p1, h, first, 7 if s else 0, other, 0)
    return out


S64 = "ACGT" * 16
S65 = S64[1:] + "GA"
# ten strings behind one column, in record order: count descending, then len, then the key
TEN = [("GG", 9), ("T", 5), ("CA", 5), (S64, 4), (S65, 3), ("A", 2), ("C", 2), ("AAA", 2), ("CCC", 1), ("GGGG", 1)]


def column(pos, depth, eq, x, dl, ins, base, **more):
    d = {"pos": pos, "depth": depth, "eq": eq, "x": list(x), "del": dl, "ins": ins, "consensus_base": base}
    d.update(more)
    return d


def listed(names=None, firsts=None):
    out = []
    for k, (s, c) in enumerate(TEN[:8]):
        e = {"seq": s[:64], "count": c}
        if len(s) > 64:
            e["len"] = len(s)
        if names is not None:
            e["first_read"] = names[firsts[k]]
        out.append(e)
    return out


def test_hla_renderer_with_a_list(pkg):
    ffi = pkg.ffi
    # column 1 is contested by a mismatch (no insertions key), column 2 by its insertions (34 runs + 1 unlisted = 35 of depth 40), column 3 by one N run alone
    a1 = table(ffi, [(40, 40, (0, 0, 0, 0), 0, 0), (40, 4, (0, 36, 0, 0), 0, 3), (40, 38, (0, 0, 0, 0), 2, 35), (1, 1, (0, 0, 0, 0), 0, 1)])
    b1 = table(ffi, [(3, 3, (0, 0, 0, 0), 0, 2)])
    sm = ffi.support_summarize
    entries = [("HLA-B", [None, ("HLA-B*07:02:01:01", "G", b1, sm(b1, 3, 3))]),
               ("HLA-A", [("HLA-A*01:01:01:01", "ACGT", a1, sm(a1, 40, 40)), None])]
    base = [(0, 100), (200, 0)]                                                  # HLA-B's consensus 2 from col 100, HLA-A's consensus 1 from col 200
    firsts = list(range(10))
    rows = [(100, "TT", 2, 11, 0), (201, "A", 3, 0, 0)]
    rows += [(202, s, c, firsts[k], 1 if k == 0 else 0) for k, (s, c) in enumerate(TEN)]
    rows += [(203, "", 0, 0, 1)]
    ins = records(ffi, rows)
    names = ["read%d" % k for k in range(12)]
    head = lambda tab, m, typed: dict(list(sm(tab, m, m).items()) + [("typed_allele", typed)])
    for with_names in (False, True):
        text = ffi.consensus_support_json(entries, insertions=ins, col_base=base, read_names=names if with_names else None)
        nm = names if with_names else None
        b_ins = [{"seq": "TT", "count": 2, "first_read": "read11"} if with_names else {"seq": "TT", "count": 2}]
        expected = {
            "HLA-A": {"consensus1": dict(head(a1, 40, "HLA-A*01:01:01:01"), contested=[
                column(1, 40, 4, (0, 36, 0, 0), 0, 3, "C"),
                column(2, 40, 38, (0, 0, 0, 0), 2, 35, "G", insertions=listed(nm, firsts), more=2, other=1),
                column(3, 1, 1, (0, 0, 0, 0), 0, 1, "T", insertions=[], other=1)])},
            "HLA-B": {"consensus2": dict(head(b1, 3, "HLA-B*07:02:01:01"), contested=[column(0, 3, 3, (0, 0, 0, 0), 0, 2, "G", insertions=b_ins)])}}
        assert text == json.dumps(expected, indent=2)
    # the 64-base string is whole, the 65-base one its first 64 and its length
    got = json.loads(text)["HLA-A"]["consensus1"]["contested"][1]["insertions"]
    assert got[3] == {"seq": S64, "count": 4, "first_read": "read3"} and got[4] == {"seq": S65[:64], "count": 3, "len": 65, "first_read": "read4"}
    # without a list, or with an empty one, the bytes are the old renderer's
    old = ffi.consensus_support_json(entries)
    assert ffi.consensus_support_json(entries, insertions=records(ffi, []), col_base=base) == old
    assert "insertions" not in old and json.loads(old)["HLA-A"]["consensus1"]["contested"][1]["ins"] == 35


def test_cyp_renderer_with_a_list(pkg):
    ffi, db = pkg.ffi, pkg.database
    d6 = table(ffi, [(40, 40, (0, 0, 0, 0), 0, 0), (40, 4, (0, 36, 0, 0), 0, 3), (40, 38, (0, 0, 0, 0), 2, 35), (1, 1, (0, 0, 0, 0), 0, 1)])
    d7 = table(ffi, [(6, 6, (0, 0, 0, 0), 0, 0), (6, 6, (0, 0, 0, 0), 0, 4)])
    call = make_call(ffi, [(CYP2D6, "4.001"), (CYP2D7, None)])
    cons, cols = ["ACGT", "TA"], [d6, d7]
    sums = [ffi.support_summarize(d6, 40, 40), ffi.support_summarize(d7, 6, 6)]
    rows = [(1, "A", 3, 0, 0)] + [(2, s, c, k, 1 if k == 0 else 0) for k, (s, c) in enumerate(TEN)] + [(3, "", 0, 0, 1), (5, "GT", 4, 2, 0)]
    ins = records(ffi, rows)
    text = db.cyp_support_json(call, cons, cols, sums, insertions=ins)
    head = lambda tab, m, typ: dict(list(ffi.support_summarize(tab, m, m).items()) + [("region_type", typ)])
    expected = {
        "0_CYP2D6*4.001": dict(head(d6, 40, "CYP2D6*4.001"), contested=[
            column(1, 40, 4, (0, 36, 0, 0), 0, 3, "C"),
            column(2, 40, 38, (0, 0, 0, 0), 2, 35, "G", insertions=listed(), more=2, other=1),
            column(3, 1, 1, (0, 0, 0, 0), 0, 1, "T", insertions=[], other=1)]),
        "1_CYP2D7": dict(head(d7, 6, "CYP2D7"), contested=[column(1, 6, 6, (0, 0, 0, 0), 0, 4, "A", insertions=[{"seq": "GT", "count": 4}])])}
    assert text == json.dumps(expected, indent=2)
    # first_read goes through the mapping records: first_pair is a record, the record names the read
    maps = [db.sp_cyp_read_mapping() for _ in range(10)]
    for k, m in enumerate(maps):
        m.read = 9 - k
    named = json.loads(db.cyp_support_json(call, cons, cols, sums, insertions=ins, mappings=maps, read_names=["r%d" % k for k in range(10)]))
    assert named["1_CYP2D7"]["contested"][0]["insertions"] == [{"seq": "GT", "count": 4, "first_read": "r7"}]
    assert db.cyp_support_json(call, cons, cols, sums, insertions=records(ffi, [])) == db.cyp_support_json(call, cons, cols, sums)

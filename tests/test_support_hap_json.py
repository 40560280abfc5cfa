"""sp_consensus_support_json_hap and sp_cyp_support_json_hap on hand-made counts and records, against a json.dumps(indent=2) statement: host only, no device is touched."""
import json

import numpy as np

import pileup_hap_ref as ref
from test_cyp_support_json import CYP2D6, CYP2D7, make_call, table


def hap_list(ffi, per_target, n_targets):
    """per_target: {target: (n_cols, n_cols_total, [(calls, count, first_pair)])} -> (HAP_DTYPE records, HAP_HEAD_DTYPE[n_targets])"""
    rows, heads = [], np.zeros(n_targets, ffi.HAP_HEAD_DTYPE)
    for t in range(n_targets):
        K, total, pats = per_target.get(t, (0, 0, []))
        heads[t] = (len(rows), len(pats), K, total, 0)
        for calls, count, first in pats:
            w = [0, 0, 0, 0]
            for k, c in enumerate(calls):
                w[k // 16] |= c << (4 * (k % 16))
            rows.append((t, K, count, first, 0, w))
    haps = np.zeros(len(rows), ffi.HAP_DTYPE)
    for k, r in enumerate(rows):
        haps[k] = r
    return haps, heads


# 17 patterns over two columns, in record order: count descending, then the pattern
SEVENTEEN = [([1, 1], 40, 0), ([3, 6], 30, 1)] + [([2 + (k % 4), 1 | (8 if k >= 8 else 0)], 15 - k if k < 14 else 1, 2 + k) for k in range(15)]


def column(pos, depth, eq, x, dl, ins, base):
    return {"pos": pos, "depth": depth, "eq": eq, "x": list(x), "del": dl, "ins": ins, "consensus_base": base}


def patterns(pats, names=None, via=None):
    out = []
    for calls, count, first in pats[:16]:
        e = {"count": count, "calls": "".join("?=ACGT-?"[c & 7] + ("+" if c & 8 else "") for c in calls)}
        if names is not None:
            e["first_read"] = names[via[first] if via else first]
        out.append(e)
    return out


def test_hla_renderer_with_a_list(pkg):
    ffi = pkg.ffi
    # HLA-A consensus 1: columns 1 and 2 contested (17 patterns); HLA-B consensus 2: one contested column but a head without columns (n_cols == 0)
    a1 = table(ffi, [(40, 40, (0, 0, 0, 0), 0, 0), (40, 4, (0, 36, 0, 0), 0, 3), (40, 10, (0, 0, 0, 0), 30, 3), (40, 40, (0, 0, 0, 0), 0, 0)])
    b1 = table(ffi, [(3, 3, (0, 0, 0, 0), 0, 2)])
    sm = ffi.support_summarize
    entries = [("HLA-B", [None, ("HLA-B*07:02:01:01", "G", b1, sm(b1, 3, 3))]),
               ("HLA-A", [("HLA-A*01:01:01:01", "ACGT", a1, sm(a1, 40, 40)), None])]
    targets = [(0, 5), (2, 0)]                                                   # HLA-B's consensus 2 is target 5, HLA-A's consensus 1 target 2
    haps, heads = hap_list(ffi, {2: (2, 2, SEVENTEEN)}, 6)
    names = ["read%d" % k for k in range(20)]
    head = lambda tab, m, typed: dict(list(sm(tab, m, m).items()) + [("typed_allele", typed)])
    for with_names in (False, True):
        text = ffi.consensus_support_json(entries, haplotypes=(haps, heads), hap_target=targets, read_names=names if with_names else None)
        hap = {"columns": [1, 2], "columns_total": 2, "patterns": patterns(SEVENTEEN, names if with_names else None), "more": 1}
        expected = {
            "HLA-A": {"consensus1": dict(head(a1, 40, "HLA-A*01:01:01:01"), contested=[column(1, 40, 4, (0, 36, 0, 0), 0, 3, "C"), column(2, 40, 10, (0, 0, 0, 0), 30, 3, "G")],
                                         haplotypes=hap)},
            "HLA-B": {"consensus2": dict(head(b1, 3, "HLA-B*07:02:01:01"), contested=[column(0, 3, 3, (0, 0, 0, 0), 0, 2, "G")])}}
        assert text == json.dumps(expected, indent=2)
    got = json.loads(text)["HLA-A"]["consensus1"]["haplotypes"]["patterns"]
    assert got[1] == {"count": 30, "calls": "C-", "first_read": "read1"} and got[10]["calls"] == "A=+" and len(got) == 16
    # the cap is visible: two of five contested columns used
    cut = hap_list(ffi, {2: (2, 5, SEVENTEEN[:2])}, 6)
    assert json.loads(ffi.consensus_support_json(entries, haplotypes=cut, hap_target=targets))["HLA-A"]["consensus1"]["haplotypes"]["columns_total"] == 5
    # without a list, or with an empty one, the bytes are the old renderer's
    old = ffi.consensus_support_json(entries)
    assert ffi.consensus_support_json(entries, haplotypes=hap_list(ffi, {}, 6), hap_target=targets) == old and "haplotypes" not in old


def test_cyp_renderer_with_a_list(pkg):
    ffi, db = pkg.ffi, pkg.database
    d6 = table(ffi, [(40, 40, (0, 0, 0, 0), 0, 0), (40, 4, (0, 36, 0, 0), 0, 3), (40, 10, (0, 0, 0, 0), 30, 3), (40, 40, (0, 0, 0, 0), 0, 0)])
    d7 = table(ffi, [(6, 6, (0, 0, 0, 0), 0, 0), (6, 6, (0, 0, 0, 0), 0, 0)])
    call = make_call(ffi, [(CYP2D6, "4.001"), (CYP2D7, None)])
    cons, cols = ["ACGT", "TA"], [d6, d7]
    sums = [ffi.support_summarize(d6, 40, 40), ffi.support_summarize(d7, 6, 6)]
    haps, heads = hap_list(ffi, {0: (2, 2, SEVENTEEN)}, 2)
    text = db.cyp_support_json(call, cons, cols, sums, haplotypes=(haps, heads))
    head = lambda tab, m, typ: dict(list(ffi.support_summarize(tab, m, m).items()) + [("region_type", typ)])
    expected = {
        "0_CYP2D6*4.001": dict(head(d6, 40, "CYP2D6*4.001"), contested=[column(1, 40, 4, (0, 36, 0, 0), 0, 3, "C"), column(2, 40, 10, (0, 0, 0, 0), 30, 3, "G")],
                               haplotypes={"columns": [1, 2], "columns_total": 2, "patterns": patterns(SEVENTEEN), "more": 1}),
        "1_CYP2D7": dict(head(d7, 6, "CYP2D7"), contested=[])}
    assert text == json.dumps(expected, indent=2)
    # first_read goes through the mapping records: first_pair is a record, the record names the read
    maps = [db.sp_cyp_read_mapping() for _ in range(20)]
    for k, m in enumerate(maps):
        m.read = 19 - k
    names = ["r%d" % k for k in range(20)]
    named = json.loads(db.cyp_support_json(call, cons, cols, sums, haplotypes=(haps, heads), mappings=maps, read_names=names))
    assert named["0_CYP2D6*4.001"]["haplotypes"]["patterns"] == patterns(SEVENTEEN, names, [19 - k for k in range(20)])
    assert db.cyp_support_json(call, cons, cols, sums, haplotypes=hap_list(ffi, {}, 2)) == db.cyp_support_json(call, cons, cols, sums)
    assert ref.text((0, 2, 30, 1, (0x63, 0, 0, 0))) == "C-"

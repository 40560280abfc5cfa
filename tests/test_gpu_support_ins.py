"""The support calls with an insertion list (sp_hla_consensus_support_ins, sp_cyp_consensus_support_ins and their cohort forms) on the capability itself: three bases
are deleted from a consensus the call returned before the support call is made, so the consensus lacks bases its own reads carry.  The column in front of the gap
then comes back contested by its insertions, and the list names exactly the three deleted bases, carried by every member that inserts there.  Fixtures: those of
tests/test_gpu_consensus_support.py (a forward-strand and a reverse-strand gene) and of tests/test_gpu_cyp_support.py."""
import ctypes as C

import numpy as np
import pytest

import pileup_ins_ref as ref
from test_gpu_consensus_support import calls  # noqa: F401  (the module's fixture)
from test_gpu_cyp_support import CONS_CAP, world  # noqa: F401

pytestmark = pytest.mark.gpu


def gap_site(s, lo):
    """the first p >= lo at which s[p:p + 3], deleted, can be put back at one place only"""
    for p in range(lo, len(s) - 4):
        if s[p] != s[p + 3] and s[p + 2] != s[p - 1]:
            return p
    raise AssertionError("no site")


def hla_string_from_the_reads(c, gene, r):
    """a record's bases fetched from the caller's reads by the arithmetic the header gives beside sp_support_ins_string: first_pair is the read, first_qpos a position
    in its gene-strand segment -- forward gene: read[seg_start + qpos, + len); reverse gene: the reverse complement of read[seg_end - qpos - len, seg_end - qpos)"""
    read, q, n = int(r["first_pair"]), int(r["first_qpos"]), int(r["len"])
    seq, lo, hi = c["reads"][read], int(c["rec"][read]["seg_start"]), int(c["rec"][read]["seg_end"])
    if c["fx"].gene_fwd[gene]:
        return seq[lo + q:lo + q + n]
    return c["synth"].revcomp(seq[hi - q - n:hi - q])


def check_planted(pkg, ins, cols, col, want):
    """the records of column `col`: the planted string first, carried by every inserting member; the column contested by its insertions"""
    mine = [r for r in ins if int(r["col"]) == col]
    assert mine, (col, [int(r["col"]) for r in ins][:20])
    first = mine[0]
    c = cols[col] if isinstance(cols, np.ndarray) else cols
    assert pkg.ffi.support_ins_string(first) == want and int(first["len"]) == 3
    assert int(first["count"]) == int(c["ins"]) and 2 * int(c["ins"]) > int(c["depth"])
    assert len(mine) == 1 and int(first["n_other"]) == 0


def test_hla_a_consensus_that_lacks_three_bases(calls, pkg):  # noqa: F811
    c = calls
    synth = c["synth"]
    for k, gene in enumerate(c["genes"]):
        call, cons1, cons2 = c["out"][k]
        p = gap_site(cons1, len(cons1) // 2)
        cut = cons1[:p] + cons1[p + 3:]
        (cols1, sm1), (cols2, sm2), ins = c["db"].consensus_support(gene, c["R"], c["rec"], c["is1"], cut, cons2, insertions=True)
        if c["fx"].gene_fwd[gene]:
            col, want = p - 1, cons1[p:p + 3]
        else:                                                               # columns and strings are on the gene strand
            col, want = len(cut) - p - 1, synth.revcomp(cons1[p:p + 3])
        check_planted(pkg, ins, cols1, col, want)
        listed = [r for r in ins if int(r["len"]) > 0]
        assert listed and all(hla_string_from_the_reads(c, gene, r) == pkg.ffi.support_ins_string(r) for r in listed)     # on both strands (the loop's two genes)
        planted = [r for r in listed if int(r["col"]) == col][0]
        assert c["is1"][int(planted["first_pair"])] and int(c["rec"][int(planted["first_pair"])]["gene"]) == gene
        assert list(pkg.ffi.support_contested(cols1)).count(col) == 1
        # the list accounts for every ins count of both tables, and without the list the call is the old one
        table = np.concatenate([cols1, cols2])
        assert ref.ins_per_column(ref.as_rows(ins)) == {j: int(x["ins"]) for j, x in enumerate(table) if int(x["ins"])}
        old = c["db"].consensus_support(gene, c["R"], c["rec"], c["is1"], cut, cons2)
        assert old[0][0].tobytes() == cols1.tobytes() and old[1][0].tobytes() == cols2.tobytes() and old[0][1] == sm1 and old[1][1] == sm2


def test_hla_cohort_form_equals_the_single_calls(calls):  # noqa: F811
    c = calls
    cons = []
    for k in range(len(c["genes"])):
        call, cons1, cons2 = c["out"][k]
        p = gap_site(cons1, len(cons1) // 2)
        cons.append((cons1[:p] + cons1[p + 3:], cons2))
    both, ins, off = c["db"].consensus_support_cohort(1, None, c["genes"], c["R"], c["rec"], c["is1"], [cons], insertions=True)
    rows = []
    for k, gene in enumerate(c["genes"]):
        single = c["db"].consensus_support(gene, c["R"], c["rec"], c["is1"], cons[k][0], cons[k][1], insertions=True)
        for side in range(2):
            assert both[0][k][side][0].tobytes() == single[side][0].tobytes() and both[0][k][side][1] == single[side][1]
        for r in ref.as_rows(single[2]):                                    # the single call numbers its two consensuses from 0; the cohort uses col_offset
            rows.append((r[0] + int(off[2 * k]),) + r[1:])
    assert ref.as_rows(ins) == rows and len(rows) >= 2


def cut_block(cons, h, p):
    """the consensus block with three bases of consensus h deleted at p"""
    raw = bytearray(cons.raw)
    text = raw[h * CONS_CAP:(h + 1) * CONS_CAP].split(b"\0", 1)[0]
    new = text[:p] + text[p + 3:]
    raw[h * CONS_CAP:(h + 1) * CONS_CAP] = new.ljust(CONS_CAP, b"\0")
    return C.create_string_buffer(bytes(raw), len(raw))


def test_cyp_a_region_that_lacks_three_bases(world, pkg, gpu_ctx):  # noqa: F811
    db = pkg.database
    s = world["samples"]["*1/*4"]
    sums = db.cyp_consensus_support(gpu_ctx, s["R"], s["call"], s["cons"], CONS_CAP, s["mappings"])[1]
    h = max(range(len(sums)), key=lambda x: sums[x]["median_depth"])
    text = s["text"][h]
    p = gap_site(text, len(text) // 2)
    block = cut_block(s["cons"], h, p)
    cols, sm, ins = db.cyp_consensus_support(gpu_ctx, s["R"], s["call"], block, CONS_CAP, s["mappings"], insertions=True)
    base = sum(len(c) for c in cols[:h])
    mine = ins[(ins["col"] >= base) & (ins["col"] < base + len(cols[h]))].copy()
    mine["col"] -= base
    check_planted(pkg, mine, cols[h], p - 1, text[p:p + 3])
    first = [r for r in mine if int(r["col"]) == p - 1][0]
    m = s["mappings"][int(first["first_pair"])]                             # first_pair is the member's mapping record, first_qpos a position in its segment
    q = int(first["first_qpos"])
    assert m.consensus == h and s["reads"][m.read][m.read_start + q:m.read_start + q + 3] == text[p:p + 3]
    for r in ins:                                                           # the header's arithmetic on every listed record
        if int(r["len"]):
            mm, qq = s["mappings"][int(r["first_pair"])], int(r["first_qpos"])
            assert s["reads"][mm.read][mm.read_start + qq:mm.read_start + qq + int(r["len"])] == pkg.ffi.support_ins_string(r)
    table = np.concatenate(cols)
    assert ref.ins_per_column(ref.as_rows(ins)) == {j: int(x["ins"]) for j, x in enumerate(table) if int(x["ins"])}
    old = db.cyp_consensus_support(gpu_ctx, s["R"], s["call"], block, CONS_CAP, s["mappings"])
    assert [c.tobytes() for c in old[0]] == [c.tobytes() for c in cols] and old[1] == sm
    # the renderer writes the planted string under the contested column
    import json
    out = json.loads(db.cyp_support_json(s["call"], [s["text"][x] if x != h else text[:p] + text[p + 3:] for x in range(len(cols))], cols, sm, insertions=ins))
    entry = [e for e in list(out.values())[h]["contested"] if e["pos"] == p - 1][0]
    assert entry["insertions"] == [{"seq": text[p:p + 3], "count": int(first["count"])}]


def test_cyp_cohort_form_equals_the_single_calls(world, pkg, gpu_ctx):  # noqa: F811
    db = pkg.database
    names = list(world["samples"])
    ss = [world["samples"][n] for n in names]
    blocks = []
    for s in ss:
        p = gap_site(s["text"][0], len(s["text"][0]) // 2)
        blocks.append(cut_block(s["cons"], 0, p))
    both, ins, off = db.cyp_consensus_support_cohort(gpu_ctx, [s["R"] for s in ss], [s["call"] for s in ss], blocks, CONS_CAP, [s["mappings"] for s in ss], insertions=True)
    rows, m0 = [], 0
    for i, s in enumerate(ss):
        cols, sm, single = db.cyp_consensus_support(gpu_ctx, s["R"], s["call"], blocks[i], CONS_CAP, s["mappings"], insertions=True)
        assert [c.tobytes() for c in both[i][0]] == [c.tobytes() for c in cols] and both[i][1] == sm
        for r in ref.as_rows(single):                                       # columns from the sample's first slot, members from its first mapping record
            rows.append((r[0] + int(off[i * pkg.ffi.SP_CYP_MAXCONS]),) + r[1:6] + ((r[6] + m0) if r[1] else 0,) + r[7:])
        m0 += len(s["mappings"])
    assert ref.as_rows(ins) == rows and len(rows) >= 2

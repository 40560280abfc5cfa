"""The support calls with a haplotype list (sp_hla_consensus_support_hap, sp_cyp_consensus_support_hap) on the fixtures of tests/test_gpu_support_ins.py: three
bases are deleted from a consensus the call returned and one base further on is changed, so every member disagrees with the consensus at two places at once.  Both
columns come back contested, and the list must say that the disagreements sit in the SAME reads: the pattern that carries both is the largest.  cols, summaries and
the insertion list are the bytes of the _ins form; the list is held to the three invariants of the header against the call's own table and summaries, and record
for record to tests/pileup_hap_ref.py over the members' own alignments (segments, anchor, sp_affine_align_batch: the composition the table tests re-derive).  The
cohort forms equal the single calls unit by unit, with the targets, heads and first_pair of the cohort's slots -- also beside a unit that is switched off."""
import numpy as np
import pytest

import pileup_hap_ref as ref
from test_gpu_consensus_support import calls  # noqa: F401  (the module's fixture)
from test_gpu_cyp_support import CONS_CAP, world  # noqa: F401
from test_gpu_support_ins import cut_block, gap_site

pytestmark = pytest.mark.gpu

SWAP = {"A": "C", "C": "G", "G": "T", "T": "A"}


def edit(text, p):
    """three bases deleted at p, the base 40 further on changed"""
    cut = text[:p] + text[p + 3:]
    q = p + 40
    return cut[:q] + SWAP[cut[q]] + cut[q + 1:], q


def check_linked(pkg, haps, heads, t, cols, summary, cols_at):
    """target t of a list: the invariants, and the largest pattern carries an insertion behind one of the given columns and a mismatch at the other"""
    rows, hd = ref.as_rows(haps), ref.as_heads(heads)
    first, n, K, total = hd[t]
    assert K >= 2 and n >= 1 and total == summary["n_contested"]
    used = [int(x) for x in pkg.ffi.support_contested(cols)][:K]
    assert all(c in used for c in cols_at)
    ka, kb = used.index(cols_at[0]), used.index(cols_at[1])
    linked = broken = 0
    for r in rows[first:first + n]:
        a, b = ref.call(r, ka), ref.call(r, kb)
        ins_a, x_b = bool(a & 8), 2 <= (b & 7) <= 5
        if ins_a and x_b:
            linked += r[2]
        elif (ins_a and (b & 7) == 1) or (x_b and a == 1):                   # one disagreement without the other, in a read that covers both
            broken += r[2]
    assert linked > 0 and linked > 10 * broken and 2 * linked > summary["median_depth"]
    assert pkg.ffi.support_hap_string(haps[first]) == ref.text(rows[first])
    return rows, hd


def test_hla_a_consensus_that_differs_from_its_reads_at_two_places(calls, pkg):  # noqa: F811
    c = calls
    for k, gene in enumerate(c["genes"]):
        call, cons1, cons2 = c["out"][k]
        p = gap_site(cons1, len(cons1) // 2)
        changed, q = edit(cons1, p)
        old = c["db"].consensus_support(gene, c["R"], c["rec"], c["is1"], changed, cons2, insertions=True)
        (cols1, sm1), (cols2, sm2), ins, (haps, heads) = c["db"].consensus_support(gene, c["R"], c["rec"], c["is1"], changed, cons2, insertions=True, haplotypes=True)
        assert old[0][0].tobytes() == cols1.tobytes() and old[1][0].tobytes() == cols2.tobytes() and (old[0][1], old[1][1]) == (sm1, sm2) and old[2].tobytes() == ins.tobytes()
        at = (p - 1, q) if c["fx"].gene_fwd[gene] else (len(changed) - p - 1, len(changed) - 1 - q)       # columns are on the gene strand
        rows, hd = check_linked(pkg, haps, heads, 0, cols1, sm1, at)
        ref.check_invariants(rows, hd, [cols1, cols2], [sm1["n_aligned"], sm2["n_aligned"]])
        assert all(c["is1"][r[3]] == (r[0] == 0) and int(c["rec"][r[3]]["gene"]) == gene for r in rows)   # first_pair is a member read of that consensus
        only = c["db"].consensus_support(gene, c["R"], c["rec"], c["is1"], changed, cons2, haplotypes=True)
        assert only[2][0].tobytes() == haps.tobytes() and only[2][1].tobytes() == heads.tobytes()


def test_cyp_a_region_that_differs_from_its_reads_at_two_places(world, pkg, gpu_ctx):  # noqa: F811
    db = pkg.database
    s = world["samples"]["*1/*4"]
    sums = db.cyp_consensus_support(gpu_ctx, s["R"], s["call"], s["cons"], CONS_CAP, s["mappings"])[1]
    h = max(range(len(sums)), key=lambda x: sums[x]["median_depth"])
    text = s["text"][h]
    p = gap_site(text, len(text) // 2)
    changed, q = edit(text, p)
    block = cut_block(s["cons"], h, p)
    raw = bytearray(block.raw)
    raw[h * CONS_CAP + q] = ord(changed[q])
    import ctypes as C
    block = C.create_string_buffer(bytes(raw), len(raw))
    old = db.cyp_consensus_support(gpu_ctx, s["R"], s["call"], block, CONS_CAP, s["mappings"], insertions=True)
    cols, sm, ins, (haps, heads) = db.cyp_consensus_support(gpu_ctx, s["R"], s["call"], block, CONS_CAP, s["mappings"], insertions=True, haplotypes=True)
    assert [x.tobytes() for x in old[0]] == [x.tobytes() for x in cols] and old[1] == sm and old[2].tobytes() == ins.tobytes()
    assert len(heads) == len(cols)
    rows, hd = check_linked(pkg, haps, heads, h, cols[h], sm[h], (p - 1, q))
    ref.check_invariants(rows, hd, cols, [x["n_aligned"] for x in sm])
    assert all(s["mappings"][r[3]].consensus == r[0] for r in rows)                                     # first_pair is a mapping record of that consensus
    # the renderer writes the list under the region
    import json
    texts = [s["text"][x] if x != h else changed for x in range(len(cols))]
    out = json.loads(db.cyp_support_json(s["call"], texts, cols, sm, haplotypes=(haps, heads)))
    entry = list(out.values())[h]["haplotypes"]
    assert entry["columns_total"] == hd[h][3] and entry["patterns"][0] == {"count": rows[hd[h][0]][2], "calls": ref.text(rows[hd[h][0]])}
    assert db.cyp_support_json(s["call"], texts, cols, sm) == db.cyp_support_json(s["call"], texts, cols, sm, haplotypes=(haps[:0], heads))


def hla_reference(c, gpu_ctx, gene, cons1, cons2):
    """the list of one gene call, re-derived as tests/test_gpu_consensus_support.py re-derives its tables: segments and consensuses on the gene strand, anchor,
    alignment on 64 diagonals (256 for a member that found nothing there), tests/pileup_hap_ref.py.  target = consensus (0 / 1), first_pair = the member read"""
    synth, fx, rec = c["synth"], c["fx"], c["rec"]
    strand = (lambda s: s) if fx.gene_fwd[gene] else synth.revcomp
    targets = [strand(x) for x in (cons1, cons2)]
    queries, side, read_of = [], [], []
    for r in np.flatnonzero((rec["status"] == 0) & (rec["gene"] == gene)):
        k = 0 if c["is1"][r] else 1
        if targets[k]:
            queries.append(strand(c["reads"][r][int(rec[r]["seg_start"]):int(rec[r]["seg_end"])]))
            side.append(k)
            read_of.append(int(r))
    live = [k for k in range(2) if targets[k]]
    T, Q = gpu_ctx.upload([targets[k] for k in live]), gpu_ctx.upload(queries)
    t_of = [live.index(k) for k in side]
    diag, votes = gpu_ctx.anchor_batch(T, Q, t_of, list(range(len(queries))))
    pairs = [(m, t_of[m], -int(diag[m])) for m in range(len(queries))]
    aln, cigar, n_cigar = gpu_ctx.affine_align(Q, T, pairs, a=1, band=64, cigar_stride=4096)
    for m in range(len(queries)):
        if votes[m] <= 0:
            n_cigar[m] = 0
        elif aln[m]["score"] <= 0 or n_cigar[m] == 0:
            a2, c2, n2 = gpu_ctx.affine_align(Q, T, [pairs[m]], a=1, band=256, cigar_stride=4096)
            aln[m], cigar[m], n_cigar[m] = a2[0], c2[0], n2[0]
    recs, heads, _ = ref.records(pairs, aln, cigar, n_cigar, queries, [len(targets[k]) for k in live], need_score=True)
    T.close()
    Q.close()
    # the compact targets back to consensus numbers: a consensus without columns has an empty head
    out_heads, at = [], 0
    for k in range(2):
        if k in live:
            out_heads.append(heads[live.index(k)])
            at = heads[live.index(k)][0] + heads[live.index(k)][1]
        else:
            out_heads.append((at, 0, 0, 0))
    return [(live[r[0]], r[1], r[2], read_of[r[3]], r[4]) for r in recs], out_heads


def cyp_reference(ctx, s, text):
    """the list of one sample, re-derived as tests/test_gpu_cyp_support.py re-derives its tables.  target = consensus h, first_pair = the member's mapping record"""
    live = [h for h in range(len(text)) if text[h]]
    record_of = [k for k, m in enumerate(s["mappings"]) if m.consensus in live]
    members = [s["mappings"][k] for k in record_of]
    queries = [s["reads"][m.read][m.read_start:m.read_end] for m in members]
    target = [live.index(m.consensus) for m in members]
    T, Q = ctx.upload([text[h] for h in live]), ctx.upload(queries)
    diag, votes = ctx.anchor_batch(T, Q, target, list(range(len(queries))))
    pairs = [(m, target[m], -int(diag[m]), 0 if votes[m] > 0 else -1) for m in range(len(queries))]
    aln, cigar, n_cigar = ctx.affine_align(Q, T, pairs, a=1, band=64, cigar_stride=4096)
    assert n_cigar.max() <= 4096
    recs, heads, _ = ref.records(pairs, aln, cigar, n_cigar, queries, [len(text[h]) for h in live], need_score=True)
    out_heads, at = [], 0
    for h in range(len(text)):
        if h in live:
            out_heads.append(heads[live.index(h)])
            at = heads[live.index(h)][0] + heads[live.index(h)][1]
        else:
            out_heads.append((at, 0, 0, 0))
    return [(live[r[0]], r[1], r[2], record_of[r[3]], r[4]) for r in recs], out_heads


def edited_hla(c):
    cons = []
    for k in range(len(c["genes"])):
        call, cons1, cons2 = c["out"][k]
        cons.append((edit(cons1, gap_site(cons1, len(cons1) // 2))[0], cons2))
    return cons


def test_hla_lists_equal_the_reference_record_for_record(calls, gpu_ctx):  # noqa: F811
    c = calls
    for k, gene in enumerate(c["genes"]):
        changed, cons2 = edited_hla(c)[k]
        haps, heads = c["db"].consensus_support(gene, c["R"], c["rec"], c["is1"], changed, cons2, haplotypes=True)[2]
        want = hla_reference(c, gpu_ctx, gene, changed, cons2)
        assert ref.as_rows(haps) == want[0] and ref.as_heads(heads) == want[1] and len(want[0]) >= 1


def test_hla_cohort_form_equals_the_single_calls(calls):  # noqa: F811
    c = calls
    cons = edited_hla(c)
    both, ins, off, (haps, heads) = c["db"].consensus_support_cohort(1, None, c["genes"], c["R"], c["rec"], c["is1"], [cons], insertions=True, haplotypes=True)
    old = c["db"].consensus_support_cohort(1, None, c["genes"], c["R"], c["rec"], c["is1"], [cons], insertions=True)
    assert old[1].tobytes() == ins.tobytes() and old[2].tobytes() == off.tobytes()
    rows, hds = [], []
    for k, gene in enumerate(c["genes"]):
        single = c["db"].consensus_support(gene, c["R"], c["rec"], c["is1"], cons[k][0], cons[k][1], haplotypes=True)
        for side in range(2):
            assert both[0][k][side][0].tobytes() == single[side][0].tobytes() and both[0][k][side][1] == single[side][1]
            assert old[0][0][k][side][0].tobytes() == single[side][0].tobytes()
        for hd in ref.as_heads(single[2][1]):                                # the single call numbers its two consensuses 0 and 1; the cohort uses the slot 2 * unit + c
            hds.append((hd[0] + len(rows),) + hd[1:])
        rows += [(r[0] + 2 * k,) + r[1:] for r in ref.as_rows(single[2][0])]
    assert ref.as_rows(haps) == rows and ref.as_heads(heads) == hds and len(rows) >= 2
    # a unit switched off: its slots have empty heads at the running record, the others keep their records
    on = np.array([0, 1], np.uint8)
    _b, _i, _o, (haps2, heads2) = c["db"].consensus_support_cohort(1, None, c["genes"], c["R"], c["rec"], c["is1"], [cons], unit_on=on, haplotypes=True)
    n0 = hds[1][0] + hds[1][1]
    assert ref.as_rows(haps2) == rows[n0:] and ref.as_heads(heads2) == [(0, 0, 0, 0), (0, 0, 0, 0)] + [(h[0] - n0,) + h[1:] for h in hds[2:]]


def edited_cyp(s):
    text = s["text"][0]
    p = gap_site(text, len(text) // 2)
    changed, q = edit(text, p)
    raw = bytearray(cut_block(s["cons"], 0, p).raw)
    raw[q] = ord(changed[q])
    import ctypes as C
    return C.create_string_buffer(bytes(raw), len(raw)), changed


def test_cyp_list_equals_the_reference_record_for_record(world, pkg, gpu_ctx):  # noqa: F811
    db = pkg.database
    for name, s in world["samples"].items():
        block, changed = edited_cyp(s)
        cols, sm, (haps, heads) = db.cyp_consensus_support(gpu_ctx, s["R"], s["call"], block, CONS_CAP, s["mappings"], haplotypes=True)
        want = cyp_reference(gpu_ctx, s, [changed] + list(s["text"][1:]))
        assert ref.as_rows(haps) == want[0] and ref.as_heads(heads) == want[1] and len(want[0]) >= 1, name


def test_cyp_cohort_form_equals_the_single_calls(world, pkg, gpu_ctx):  # noqa: F811
    db, M = pkg.database, pkg.ffi.SP_CYP_MAXCONS
    ss = [world["samples"][n] for n in world["samples"]]
    blocks = [edited_cyp(s)[0] for s in ss]
    both, ins, off, (haps, heads) = db.cyp_consensus_support_cohort(gpu_ctx, [s["R"] for s in ss], [s["call"] for s in ss], blocks, CONS_CAP, [s["mappings"] for s in ss], haplotypes=True)
    assert ins is None and len(heads) == len(ss) * M
    rows, hds, m0 = [], [], 0
    for i, s in enumerate(ss):
        cols, sm, (h1, hd1) = db.cyp_consensus_support(gpu_ctx, s["R"], s["call"], blocks[i], CONS_CAP, s["mappings"], haplotypes=True)
        assert [c.tobytes() for c in both[i][0]] == [c.tobytes() for c in cols] and both[i][1] == sm
        base = len(rows)
        single_heads = ref.as_heads(hd1)
        for h in range(M):                                                   # slots from the sample's first, members from its first mapping record
            hds.append((single_heads[h][0] + base,) + single_heads[h][1:] if h < len(single_heads) else (len(rows) + len(h1), 0, 0, 0))
        rows += [(r[0] + i * M, r[1], r[2], r[3] + m0, r[4]) for r in ref.as_rows(h1)]
        m0 += len(s["mappings"])
    assert ref.as_rows(haps) == rows and ref.as_heads(heads) == hds and len(rows) >= 2 and len(ss) >= 2

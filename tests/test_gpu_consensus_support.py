"""sp_hla_consensus_support(_cohort): the pileup of the member reads of each consensus of an HLA gene call, against tests/pileup_ref.py over alignments this test
derives itself (sp_anchor_batch + sp_affine_align_batch on 64, then 256 diagonals) from the call's is_cons1, segments and consensuses -- on a forward-strand and on a
reverse-strand gene, single call and cohort form."""
import json

import numpy as np
import pytest

import pileup_ref as pr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def calls(pkg, gpu_ctx):
    from pb_starphase_amd import synth
    fx = synth.HlaFixture(max_alleles_per_gene=40, seed=7)
    db = fx.make_db(pkg, gpu_ctx)
    rng = np.random.default_rng(11)
    fwd = [g for g in range(len(fx.genes)) if fx.gene_fwd[g] and fx.full_length_alleles(g)][0]
    rev = [g for g in range(len(fx.genes)) if not fx.gene_fwd[g] and fx.full_length_alleles(g)][0]
    reads = []
    for g, n in ((fwd, 9), (rev, 14)):
        a = fx.full_length_alleles(g)[0]
        hap, s = fx.haplotype(g, a)
        reads += synth.simulate_reads(rng, hap, s, len(fx.dna[a]), n, mean_len=6000, sd_len=800)
    R = gpu_ctx.upload(reads)
    rec = db.realign_reads(R)
    genes = [fwd, rev]
    out, is1 = db.diplotype_genes(genes, R, rec)
    yield dict(fx=fx, db=db, genes=genes, reads=reads, R=R, rec=rec, out=out, is1=is1, synth=synth)
    R.close()
    db.close()


def expected(c, gpu_ctx, gene, cons1, cons2):
    """the tables and summaries of one gene call, re-derived: segments and consensuses on the gene strand, anchor, alignment, reference pileup"""
    synth, fx, rec = c["synth"], c["fx"], c["rec"]
    strand = (lambda s: s) if fx.gene_fwd[gene] else synth.revcomp
    targets = [strand(x) for x in (cons1, cons2)]
    queries, side = [], []
    for r in np.flatnonzero((rec["status"] == 0) & (rec["gene"] == gene)):
        k = 0 if c["is1"][r] else 1
        if targets[k]:
            queries.append(strand(c["reads"][r][int(rec[r]["seg_start"]):int(rec[r]["seg_end"])]))
            side.append(k)
    live = [k for k in range(2) if targets[k]]
    T, Q = gpu_ctx.upload([targets[k] for k in live]), gpu_ctx.upload(queries)
    t_of = [live.index(k) for k in side]
    diag, votes = gpu_ctx.anchor_batch(T, Q, t_of, list(range(len(queries))))
    pairs = [(m, t_of[m], -int(diag[m])) for m in range(len(queries))]
    aln, cigar, n_cigar = gpu_ctx.affine_align(Q, T, pairs, a=1, band=64, cigar_stride=4096)
    for m in range(len(queries)):
        if votes[m] <= 0:
            n_cigar[m] = 0
        elif aln[m]["score"] <= 0:
            a2, c2, n2 = gpu_ctx.affine_align(Q, T, [pairs[m]], a=1, band=256, cigar_stride=4096)
            aln[m], cigar[m], n_cigar[m] = a2[0], c2[0], n2[0]
    tabs = pr.pileup(queries, [len(targets[k]) for k in live], pairs, aln, cigar, n_cigar)
    res = []
    for k in range(2):
        if k not in live:
            res.append((np.zeros((0, 8), np.int64), pr.summary(np.zeros((0, 8), np.int64), 0, 0)))
            continue
        members = [m for m in range(len(queries)) if side[m] == k]
        res.append((tabs[live.index(k)], pr.summary(tabs[live.index(k)], len(members), sum(int(n_cigar[m]) > 0 for m in members))))
    T.close()
    Q.close()
    return res


def test_gene_call_support_equals_the_reference(calls, gpu_ctx, pkg):
    c = calls
    strands = set()
    for k, gene in enumerate(c["genes"]):
        call, cons1, cons2 = c["out"][k]
        assert call.status == 0 and cons1
        strands.add(bool(c["fx"].gene_fwd[gene]))
        got = c["db"].consensus_support(gene, c["R"], c["rec"], c["is1"], cons1, cons2)
        want = expected(c, gpu_ctx, gene, cons1, cons2)
        for side in range(2):
            cols, sm = got[side]
            tab = pr.as_table(cols)
            assert tab.shape == want[side][0].shape and (tab == want[side][0]).all(), (gene, side)
            assert sm == want[side][1], (gene, side, sm, want[side][1])
            assert (tab[:, 0] == tab[:, 1] + tab[:, 2:6].sum(axis=1) + tab[:, 6]).all()
            assert list(pkg.ffi.support_contested(cols)) == pr.contested(tab) and sm["n_contested"] == len(pr.contested(tab))
        assert got[0][1]["n_aligned"] >= 3 and got[0][1]["median_depth"] >= 3                # the members do pile up under their consensus
    assert strands == {True, False}


def test_cohort_form_equals_the_single_calls(calls):
    c = calls
    cons = [[(c["out"][k][1], c["out"][k][2]) for k in range(len(c["genes"]))]]
    both = c["db"].consensus_support_cohort(1, None, c["genes"], c["R"], c["rec"], c["is1"], cons)
    for k, gene in enumerate(c["genes"]):
        single = c["db"].consensus_support(gene, c["R"], c["rec"], c["is1"], cons[0][k][0], cons[0][k][1])
        for side in range(2):
            assert both[0][k][side][0].tobytes() == single[side][0].tobytes() and both[0][k][side][1] == single[side][1]
    # a unit switched off gets no columns and a zeroed summary; the other is unchanged
    off = c["db"].consensus_support_cohort(1, None, c["genes"], c["R"], c["rec"], c["is1"], cons, unit_on=[0, 1])
    assert len(off[0][0][0][0]) == 0 and off[0][0][0][1]["n_members"] == 0
    assert off[0][1][0][0].tobytes() == both[0][1][0][0].tobytes()


def test_cohort_of_two_samples_equals_each_sample_alone(calls, gpu_ctx):
    """two samples in one read set (the second: the same reads without every fifth one, in another order): read_sample, the sample-major units and the per-unit
    switch of the cohort form against the single-sample call on each sample's own reads"""
    c, db, genes = calls, calls["db"], calls["genes"]
    second = [r for i, r in enumerate(c["reads"]) if i % 5 != 2][::-1]
    both = c["reads"] + second
    read_sample = [0] * len(c["reads"]) + [1] * len(second)
    R = gpu_ctx.upload(both)
    rec = db.realign_reads(R)
    out, is1 = db.diplotype_cohort(2, read_sample, genes, R, rec, cap=65536)
    cons = [[(out[s][k][1], out[s][k][2]) for k in range(len(genes))] for s in range(2)]
    got = db.consensus_support_cohort(2, read_sample, genes, R, rec, is1, cons)
    off = db.consensus_support_cohort(2, read_sample, genes, R, rec, is1, cons, unit_on=[1, 0, 0, 1])
    for s, reads in enumerate((c["reads"], second)):
        Rs = gpu_ctx.upload(reads)
        recs = db.realign_reads(Rs)
        alone, is1s = db.diplotype_genes(genes, Rs, recs)
        for k, gene in enumerate(genes):
            assert (alone[k][1], alone[k][2]) == cons[s][k]
            single = db.consensus_support(gene, Rs, recs, is1s, alone[k][1], alone[k][2])
            for side in range(2):
                assert got[s][k][side][0].tobytes() == single[side][0].tobytes() and got[s][k][side][1] == single[side][1], (s, k, side)
                want = single[side] if (s, k) in ((0, 0), (1, 1)) else None
                if want is None:
                    assert len(off[s][k][side][0]) == 0 and off[s][k][side][1]["n_members"] == 0
                else:
                    assert off[s][k][side][0].tobytes() == want[0].tobytes() and off[s][k][side][1] == want[1]
            assert got[s][k][0][1]["n_members"] > 0
        Rs.close()
    R.close()


# ------------------------------------------------------------------ the designed sample: a substitution planted in a known share of one consensus's members
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def designed_reads(fx, synth, gene, share, n=10, seed=23):
    """error-free reads of one allele of `gene`; the members that span the chosen column are counted and `share` of them get another base there.
    -> (reads, the 25-mer around the column in hg38 orientation, original base, planted base, spanning members, planted members)"""
    rng = np.random.default_rng(seed)
    a = fx.full_length_alleles(gene)[0]
    hap, s = fx.haplotype(gene, a)
    reads = synth.simulate_reads(rng, hap, s, len(fx.dna[a]), n, mean_len=6000, sd_len=800, errors=False)
    best = None
    for p in range(s + 300, s + len(fx.dna[a]) - 300, 97):
        kmer = hap[p - 12:p + 13]
        if hap.count(kmer) != 1:
            continue
        span = [i for i, r in enumerate(reads) if kmer in r]
        if best is None or len(span) > len(best[1]):
            best = (p, span, kmer)
        if len(span) == n:
            break
    p, span, kmer = best
    orig = hap[p]
    plant = "ACGT"[("ACGT".index(orig) + 2) % 4]
    n_plant = int(round(share * len(span)))
    out = list(reads)
    for i in span[:n_plant]:
        at = out[i].index(kmer) + 12
        out[i] = out[i][:at] + plant + out[i][at + 1:]
    return out, kmer, orig, plant, len(span), n_plant


def searched_base(oracle, reads, kmer, plant):
    """CPU pre-check: the single consensus (ConsensusDWFA of a read group, the library's oracle/ statement of it) over the 325-base windows of the spanning members
    around the column -> the base the search puts on the column"""
    import oracle_ffi as of
    windows = []
    for r in reads:
        for k in (kmer, kmer[:12] + plant + kmer[13:]):
            at = r.find(k)
            if at >= 150 and at + 175 <= len(r):
                windows.append(r[at - 150:at + 175])
    res = of.oracle_consensus(oracle, windows, cfg=of.cons_config(dual=False))
    assert not res["gave_up"] and len(res["cons"][0]) >= 200
    return res["cons"][0][162], len(windows)


def test_designed_sample_one_contested_column(calls, gpu_ctx, pkg, oracle):
    """A substitution planted in 60 % of the members of one consensus (reverse-strand gene, error-free reads of the consensus's allele) makes exactly that column
    contested, with x[planted base] equal to the planted count; planted in 30 % the list is empty.

    The CPU pre-check the design asks for was run first (searched_base, asserted below): at 60 % the consensus search does NOT keep the unplanted base -- a read
    group's consensus follows the majority of its members, so a consensus searched from the planted reads carries the planted base, and then 60 % of the members
    agree with it and no column is contested, whichever way the plant points.  A column is contested only against a consensus that a majority of its spanning
    members contradicts.  So the plant is made in the non-majority direction of the search: the consensus handed to sp_hla_consensus_support is the one the call
    gives for the SAME members before the plant (the allele they were synthesised from), and is_cons1 names every read a member of it; the planted reads are
    realigned by K1 themselves."""
    c, db, fx, synth = calls, calls["db"], calls["fx"], calls["synth"]
    gene = c["genes"][1]
    assert not fx.gene_fwd[gene]
    clean, kmer, orig, plant, n_span, _ = designed_reads(fx, synth, gene, 0.0)
    Rc = gpu_ctx.upload(clean)
    (call, cons1, cons2), = db.diplotype_genes([gene], Rc, db.realign_reads(Rc))[0]
    Rc.close()
    assert call.status == 0 and not call.is_dual and cons1.count(kmer) == 1 and n_span >= 5
    q = cons1.index(kmer) + 12                                   # the column on the hg38-forward consensus
    pos = len(cons1) - 1 - q                                     # ... and on the gene strand
    strand_cons = synth.revcomp(cons1)
    assert strand_cons[pos] == COMP[orig]
    for share, contested in ((0.6, True), (0.3, False)):
        reads, _k, _o, _p, n_span2, n_plant = designed_reads(fx, synth, gene, share)
        assert n_span2 == n_span and 0 < n_plant < n_span and (2 * (n_span - n_plant) <= n_span) == contested
        base, n_win = searched_base(oracle, reads, kmer, plant)
        assert n_win >= 5
        if contested:
            assert base == plant                                  # the pre-check: the search flips to the planted base at 60 % (see the docstring)
        else:
            assert base == orig
        R = gpu_ctx.upload(reads)
        rec = db.realign_reads(R)
        assert ((rec["status"] == 0) & (rec["gene"] == gene)).all()
        (cols, sm), (cols2, sm2) = db.consensus_support(gene, R, rec, np.ones(len(reads), np.uint8), cons1, "")
        R.close()
        assert sm["n_members"] == sm["n_aligned"] == len(reads) and sm["length"] == len(cons1) and len(cols2) == 0
        tab = pr.as_table(cols)
        assert tab[pos][0] == n_span and tab[pos][1] == n_span - n_plant and tab[pos][6] == 0 and tab[pos][7] == 0
        x = [0, 0, 0, 0]
        x["ACGT".index(COMP[plant])] = n_plant                    # the planted base as the gene strand reads it
        assert list(tab[pos][2:6]) == x
        assert list(pkg.ffi.support_contested(cols)) == ([pos] if contested else []) and sm["n_contested"] == int(contested)
        other = np.delete(tab, pos, axis=0)
        assert (other[:, 0] == other[:, 1]).all() and (other[:, 7] == 0).all()                  # everywhere else every spanning member agrees
        doc = json.loads(pkg.ffi.consensus_support_json([(fx.genes[gene], [("typed", strand_cons, cols, sm), None])]))
        want = [dict(pos=pos, depth=n_span, eq=n_span - n_plant, x=x, ins=0, consensus_base=COMP[orig], **{"del": 0})] if contested else []
        assert doc[fx.genes[gene]]["consensus1"]["contested"] == want

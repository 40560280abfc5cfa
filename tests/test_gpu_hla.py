"""GPU parity for the fused HLA entry points (K1 sp_hla_realign_reads, K2 sp_hla_score_consensus)."""
import numpy as np
import pytest

import hla_expected as hx
import oracle_ffi as of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small(pkg, gpu_ctx):
    from pb_starphase_amd import synth
    fx = synth.HlaFixture(max_alleles_per_gene=90, seed=2)
    db = fx.make_db(pkg, gpu_ctx)
    yield fx, db
    db.close()


def test_k2_score_consensus(oracle, pkg, gpu_ctx, small):
    from pb_starphase_amd import synth
    fx, db = small
    rng = np.random.default_rng(4)
    for g in range(len(fx.genes)):
        cands = [a for a in range(len(fx.ids)) if fx.gene_of[a] == g and fx.dna[a]]
        for trial, a in enumerate(rng.choice(cands, 3, replace=False).tolist()):
            # consensus = the allele inside a little reference flank (gene strand), plus a few edits on later trials
            ref = fx.gene_ref[g] if fx.gene_fwd[g] else synth.revcomp(fx.gene_ref[g])
            dna = ref[:60] + fx.dna[a] + ref[-60:]
            cdna = fx.cdna[a]
            if trial == 1:
                dna = synth.mutate(rng, dna, 2, 1, 1)
                cdna = synth.mutate(rng, cdna, 1, 0, 0)
            if trial == 2:
                cdna = cdna[5:-7]
            for require_dna in (False, True):
                best, n_scored, stats = db.score_consensus(g, dna, cdna, require_dna=require_dna)
                ebest, estats = hx.k2_expected(oracle, fx, g, dna, cdna, require_dna=require_dna)
                assert n_scored == len(estats)
                assert best == ebest, (fx.ids[best] if best >= 0 else None, fx.ids[ebest] if ebest >= 0 else None)
                for al, st in estats.items():
                    assert stats[al].tolist() == st, (al, stats[al], st)
                if trial == 0:
                    assert best == a or fx.cdna[best] == fx.cdna[a]
    # nothing maps: 4-bp consensus (reference: test_score_bad_read, src/hla/caller.rs:1784-1809)
    best, n_scored, stats = db.score_consensus(0, "ACGT", "N", require_dna=True, disable_cdna=True)
    assert best == -1
    assert all(s == [-1] * 6 for s in stats[[a for a in range(len(fx.ids)) if fx.gene_of[a] == 0 and fx.dna[a]]].tolist())


def test_k1_realign_reads(oracle, pkg, gpu_ctx, small, k1_exhaustive):
    from pb_starphase_amd import synth
    fx, db = small
    rng = np.random.default_rng(9)
    reads = []
    for g in range(len(fx.genes)):
        full = fx.full_length_alleles(g)
        for a in rng.choice(full, 2, replace=False).tolist():
            hap, gs = fx.haplotype(g, a)
            reads += synth.simulate_reads(rng, hap, gs, len(fx.dna[a]), 5, mean_len=6500, sd_len=1200)
    # noisy reads: the accepted allele has > 8 and > 32 edits, so the deeper passes of the pruned mode are exercised
    reads.append(synth.mutate(rng, reads[1], 20, 10, 10))
    reads.append(synth.mutate(rng, reads[12], 60, 35, 35))
    reads.append(synth.mutate(rng, reads[7], 150, 60, 60))          # beyond the 3 % cut-off
    reads.append("".join(rng.choice(list("ACGT"), 5000)))          # junk read: no allele
    reads.append(reads[0][:3100])                                    # truncated read
    reads.append(reads[2][len(reads[2]) - 2600:])                    # starts inside the alleles: negative band diagonals (no snapshot / resume)
    reads.append(reads[6][1500:1500 + 3000])
    rs = gpu_ctx.upload(reads)
    out, cells = db.realign_reads(rs, cells=True)
    exp, ecells = hx.k1_expected(oracle, fx, reads)
    assert (cells == ecells).all(), np.argwhere(cells != ecells)[:10]
    n_real = 0
    for r, e in enumerate(exp):
        o = out[r]
        assert o["status"] == e["status"], (r, o, e)
        assert o["best_allele"] == e["best_allele"], (r, o, e)
        if e["best_allele"] >= 0:
            assert o["gene"] == e["gene"]
            assert (o["nm"], o["target_len"], o["unmapped"]) == (e["nm"], e["target_len"], e["unmapped"])
            assert tuple(int(x) for x in o["aln"].tolist()) == e["aln"]
            # the winner re-scored the reference's way: (score, NM, allele span, read span) of the two-piece affine local alignment
            assert (o["mm2_score"], o["mm2_nm"], o["mm2_t_start"], o["mm2_t_end"], o["mm2_q_start"], o["mm2_q_end"]) == e["mm2"], (r, o, e["mm2"])
            assert e["mm2"][0] > 0 and abs(e["mm2"][1] - e["nm"]) <= 3
        else:
            assert o["mm2_score"] == 0
        if e["status"] == 0:
            n_real += 1
            assert (o["seg_start"], o["seg_end"], o["dna_offset"], o["hpc_offset"]) == \
                   (e["seg_start"], e["seg_end"], e["dna_offset"], e["hpc_offset"]), (r, o, e)
    assert n_real >= len(reads) - 7
    assert out[len(reads) - 4]["best_allele"] == -1
    # production mode (no cell matrix requested): exact branch-and-bound must not change a single output field
    for _ in range(3):
        pruned = db.realign_reads(rs)
        assert pruned.tobytes() == out.tobytes()


def test_k1_reads_with_n(oracle, pkg, gpu_ctx, small, k1_exhaustive):
    """reads carrying N bases take the N-plane variants of every K1 kernel (an N never matches, not even another N)"""
    from pb_starphase_amd import synth
    fx, db = small
    rng = np.random.default_rng(21)
    reads = []
    for g in range(len(fx.genes)):
        a = int(rng.choice(fx.full_length_alleles(g)))
        hap, gs = fx.haplotype(g, a)
        reads += synth.simulate_reads(rng, hap, gs, len(fx.dna[a]), 4, mean_len=6500, sd_len=1200)
    for r in (0, 3, 5):
        s = list(reads[r])
        for p in rng.choice(len(s), 6, replace=False):
            s[int(p)] = "N"
        reads[r] = "".join(s)
    reads[1] = reads[1][:2000] + "N" * 40 + reads[1][2040:]          # a run of N: more edits than the first pass allows
    rs = gpu_ctx.upload(reads)
    out, cells = db.realign_reads(rs, cells=True)
    exp, ecells = hx.k1_expected(oracle, fx, reads)
    assert (cells == ecells).all(), np.argwhere(cells != ecells)[:10]
    for r, e in enumerate(exp):
        assert out[r]["status"] == e["status"] and out[r]["best_allele"] == e["best_allele"], (r, out[r], e)
        if e["best_allele"] >= 0:
            assert (out[r]["nm"], out[r]["target_len"], out[r]["unmapped"]) == (e["nm"], e["target_len"], e["unmapped"])
    assert db.realign_reads(rs).tobytes() == out.tobytes()


class _SyntheticGene:
    """a one-gene database of long alleles in the shape HlaFixture hands to the library and to hla_expected"""
    def __init__(self, rng, synth, ref_len=7600, n_alleles=40):
        self.genes, self.buffer = ["SYN-1"], 100
        ref = "".join(rng.choice(list("ACGT"), ref_len))
        self.gene_ref, self.gene_fwd = [ref], [1]
        core = ref[300:ref_len - 300]                                 # 7,000 bases: beyond the 5,088 the register prefetch covers
        self.exons = [[(400, 700), (1500, 1800), (3000, 3300)]]
        self.dna, self.cdna, self.ids = [], [], []
        base_variants = [core]
        for k in range(n_alleles - 1):
            parent = base_variants[int(rng.integers(0, len(base_variants)))]
            child = synth.mutate(rng, parent, int(rng.integers(1, 5)), int(rng.integers(0, 2)), int(rng.integers(0, 2)))
            base_variants.append(child)
        for k, seq in enumerate(base_variants):
            if k % 9 == 4:
                seq = seq[:int(rng.integers(2500, 4800))]            # a few partial alleles: mixed fast / direct staging in one group
            self.ids.append(f"SYN{k:04d}")
            self.dna.append(seq)
            self.cdna.append(seq[100:400] + seq[1200:1500])
        self.gene_of = np.zeros(len(self.ids), np.uint32)

    def dna_fwd(self, a):
        return self.dna[a]


def test_k1_long_alleles(oracle, pkg, gpu_ctx, k1_exhaustive):
    """alleles longer than the fixed-shape register prefetch (5,088 bases) go through the direct staging path of k1_cells and
    through cooperative extensions of several thousand bases"""
    from pb_starphase_amd import synth
    rng = np.random.default_rng(31)
    fx = _SyntheticGene(rng, synth)
    db = pkg.HlaDb(gpu_ctx, fx.gene_of, fx.dna, fx.cdna, fx.gene_ref, fx.gene_fwd, fx.exons, fx.buffer)
    reads = []
    for a in (0, 7, 13, 22, 31):
        hap = fx.gene_ref[0][:300] + fx.dna[a] + fx.gene_ref[0][300 + len(fx.dna[a]):] if len(fx.dna[a]) > 6000 else fx.gene_ref[0]
        reads.append(synth.hifi_errors(rng, hap))
        reads.append(synth.hifi_errors(rng, hap[150:-200]))
    reads.append(synth.mutate(rng, reads[0], 30, 12, 12))
    rs = gpu_ctx.upload(reads)
    out, cells = db.realign_reads(rs, cells=True)
    exp, ecells = hx.k1_expected(oracle, fx, reads)
    assert (cells == ecells).all(), np.argwhere(cells != ecells)[:10]
    for r, e in enumerate(exp):
        assert out[r]["status"] == e["status"] and out[r]["best_allele"] == e["best_allele"], (r, out[r], e)
        if e["best_allele"] >= 0:
            assert (out[r]["nm"], out[r]["target_len"], out[r]["unmapped"]) == (e["nm"], e["target_len"], e["unmapped"])
    assert (out["status"] == 0).sum() >= len(reads) - 2
    assert db.realign_reads(rs).tobytes() == out.tobytes()
    db.close()


def test_k1_synthetic_fuzz(oracle, pkg, gpu_ctx, k1_exhaustive):
    """random one-gene databases whose alleles descend from each other (rich shared-prefix structure: chains, snapshots, resumes),
    clean / noisy / partial reads; the whole cell matrix and every output field against the oracle.  SP_FUZZ_SEEDS widens the hunt."""
    import os
    from pb_starphase_amd import synth
    for seed in [int(x) for x in os.environ.get("SP_FUZZ_SEEDS", "5,6").split(",")]:
        rng = np.random.default_rng(1000 + seed)
        ref_len = int(rng.choice([1400, 2600, 4200]))
        fx = _SyntheticGene(rng, synth, ref_len=ref_len, n_alleles=int(rng.integers(70, 200)))
        db = pkg.HlaDb(gpu_ctx, fx.gene_of, fx.dna, fx.cdna, fx.gene_ref, fx.gene_fwd, fx.exons, fx.buffer)
        reads = []
        for a in rng.choice(len(fx.ids), 6, replace=False).tolist():
            full = len(fx.dna[a]) > ref_len - 700
            hap = fx.gene_ref[0][:300] + fx.dna[a] + fx.gene_ref[0][300 + len(fx.dna[a]):] if full else fx.gene_ref[0]
            reads.append(synth.hifi_errors(rng, hap))
            reads.append(hap)                                          # error free: bound 0, every other allele cut at once
            cut = int(rng.integers(100, 500))
            reads.append(synth.hifi_errors(rng, hap[cut:]))
        reads.append(synth.mutate(rng, reads[0], 14, 5, 5))
        rs = gpu_ctx.upload(reads)
        out, cells = db.realign_reads(rs, cells=True)
        exp, ecells = hx.k1_expected(oracle, fx, reads)
        assert (cells == ecells).all(), (seed, np.argwhere(cells != ecells)[:10])
        for r, e in enumerate(exp):
            assert out[r]["status"] == e["status"] and out[r]["best_allele"] == e["best_allele"], (seed, r, out[r], e)
            if e["best_allele"] >= 0:
                assert (out[r]["nm"], out[r]["target_len"], out[r]["unmapped"]) == (e["nm"], e["target_len"], e["unmapped"])
        assert db.realign_reads(rs).tobytes() == out.tobytes(), seed
        db.close()


def test_type_consensus(oracle, pkg, gpu_ctx, small):
    """sp_hla_type_consensus = score_consensus + splice_read (src/hla/caller.rs:1258-1319,1518-1576): the hg38-forward
    consensus goes in, the library places it on the gene reference, splices the cDNA and types it."""
    from pb_starphase_amd import synth
    fx, db = small
    rng = np.random.default_rng(21)
    for g in range(len(fx.genes)):
        full = fx.full_length_alleles(g)
        for trial, a in enumerate(rng.choice(full, 2, replace=False).tolist()):
            hap, s = fx.haplotype(g, a)
            cons = hap[max(0, s - 150):s + len(fx.dna[a]) + 150]
            if trial == 1:
                cons = synth.mutate(rng, cons, 2, 1, 1)
            best, n_scored, stats, cdna = db.type_consensus(g, cons)
            # expected, step by step with the oracle
            ref = fx.gene_ref[g][fx.buffer:len(fx.gene_ref[g]) - fx.buffer]
            d, v = oracle.anchor(fx.gene_ref[g], cons)                     # cons_pos - ref_pos (buffered reference)
            assert v >= 2
            al, ev = oracle.wfa(cons, ref, -d - fx.buffer, retry=2)
            assert al.ok
            cigar = oracle.cigar(al, ev)
            bam = [(l, {7: 0, 8: 0, 1: 1, 2: 2}[op]) for l, op in cigar]
            if al.a_start:
                bam.insert(0, (al.a_start, 4))
            exons = [(e0 - fx.buffer, e1 - fx.buffer) for e0, e1 in fx.exons[g]]
            segs, _ = oracle.splice_read(al.b_start, bam, exons)
            spliced = "".join(cons[x:y] for x, y in segs)
            fwd = bool(fx.gene_fwd[g])
            e_dna = cons if fwd else synth.revcomp(cons)
            e_cdna = spliced if fwd else synth.revcomp(spliced)
            assert cdna == e_cdna
            ebest, estats = hx.k2_expected(oracle, fx, g, e_dna, e_cdna)
            assert best == ebest and n_scored == len(estats)
            for al_i, st in estats.items():
                assert stats[al_i].tolist() == st
            # the winner's stats re-scored the reference's way (sp_hla_best.mm2_stats; a = 5): oracle/affine.c of the allele (query) on the consensus (target)
            want = []
            for seq_a, seq_c in ((fx.cdna[best], e_cdna), (fx.dna[best], e_dna)):
                if not seq_a or not seq_c:
                    want += [-1, -1, -1]
                    continue
                dd, _vv = oracle.anchor(seq_a, seq_c)                       # cons_pos - allele_pos
                sc, nm2, _ts, _te, qs, qe = of.oracle_affine(oracle, seq_c, seq_a, -dd, 64, 5)
                want += [len(seq_a), nm2, len(seq_a) - (qe - qs)] if sc > 0 else [-1, -1, -1]
            assert db.last_mm2_stats == want, (db.last_mm2_stats, want, stats[best].tolist())
            if trial == 0:
                assert best == a or (fx.cdna[best] == fx.cdna[a] and fx.dna[best] == fx.dna[a])
    # empty / unalignable consensus => unknown (caller.rs:1263-1267,1282-1287)
    assert db.type_consensus(0, "")[0:2] == (-1, 0)
    junk = "".join(rng.choice(list("ACGT"), 3000))
    assert db.type_consensus(0, junk)[0] == -1


def test_k1_full_database_pruned_equals_exhaustive(oracle, pkg, gpu_ctx, k1_exhaustive):
    """BASELINE configs[1] shape at reduced read count: the full bundled IMGT/HLA database (18,461 alleles), 240 synthetic HiFi
    reads.  Size-independent properties: the production (branch-and-bound + iterative deepening) mode must reproduce the
    exhaustive mode byte for byte, every read must land in its gene, and a sample of reads is checked against the oracle."""
    import ctypes as C
    from pb_starphase_amd import synth
    fx = synth.HlaFixture()
    db = fx.make_db(pkg, gpu_ctx)
    wl = synth.Config2Workload(fx, n_reads=240, seed=77)
    rng = np.random.default_rng(5)
    reads = list(wl.reads)
    for i in (3, 50, 101):                                     # noisy reads that need the deeper passes
        reads[i] = synth.mutate(rng, reads[i], 25, 12, 12)
    rs = gpu_ctx.upload(reads)
    full, cells = db.realign_reads(rs, cells=True)
    for _ in range(2):
        assert db.realign_reads(rs).tobytes() == full.tobytes()
    assert all(full[r]["gene"] == wl.read_truth[r][0] for r in range(len(reads)) if full[r]["status"] == 0)
    assert (full["status"] == 0).mean() > 0.97
    # oracle spot check (whole-read K1 search in C)
    L = oracle.L
    L.osp_hla_k1_read.restype = C.c_int32
    refs = [oracle.encode(s) for s in fx.gene_ref]
    enc = [oracle.encode(fx.dna_fwd(a)) if fx.dna[a] else np.zeros(0, np.uint8) for a in range(len(fx.ids))]
    off = np.full(len(fx.ids), -2 ** 31, np.int32)
    for a in range(len(fx.ids)):
        if len(enc[a]):
            d, v = oracle.anchor(refs[int(fx.gene_of[a])], enc[a])
            if v >= 16:
                off[a] = d
    ref_ptr = (C.c_void_p * len(refs))(*[r.ctypes.data for r in refs])
    ref_len = np.array([len(r) for r in refs], np.int32)
    al_ptr = (C.c_void_p * len(enc))(*[(e.ctypes.data if len(e) else None) for e in enc])
    al_len = np.array([len(e) for e in enc], np.int32)
    gene_of = fx.gene_of.astype(np.int32)
    for r in (0, 3, 17, 50, 199):
        re = oracle.encode(reads[r])
        ecell = np.zeros(len(fx.ids), np.uint32)
        nrun = C.c_int64(0)
        b = L.osp_hla_k1_read(re.ctypes.data_as(C.c_void_p), len(re), len(refs), ref_ptr, ref_len.ctypes.data_as(C.c_void_p), len(enc), al_ptr,
                              al_len.ctypes.data_as(C.c_void_p), gene_of.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p),
                              ecell.ctypes.data_as(C.c_void_p), C.byref(nrun))
        assert b == full[r]["best_allele"]
        assert (cells[r] == ecell).all()
    db.close()


def test_k2_batch_equals_single(oracle, pkg, gpu_ctx, small):
    """sp_hla_score_consensus_batch / sp_hla_type_consensus_batch: the batched launches give what the single calls give"""
    from pb_starphase_amd import synth
    fx, db = small
    rng = np.random.default_rng(8)
    items, fwd_items = [], []
    for g in range(len(fx.genes)):
        for a in rng.choice(fx.full_length_alleles(g), 3, replace=False).tolist():
            hap, s = fx.haplotype(g, a)
            cons = synth.mutate(rng, hap[max(0, s - 120):s + len(fx.dna[a]) + 120], 2, 1, 0)
            fwd_items.append((g, cons))
            items.append((g, synth.mutate(rng, fx.dna[a], 1, 1, 0), fx.cdna[a]))
    fwd_items.append((0, ""))                                       # failed consensus => unknown
    fwd_items.append((1, "".join(rng.choice(list("ACGT"), 2500))))  # does not align => unknown
    single = [db.score_consensus(g, d, c, stats=False)[:2] for g, d, c in items]
    assert db.score_consensus_batch(items) == [(b, n) for b, n in single]
    single_t = [db.type_consensus(g, c, stats=False)[:2] for g, c in fwd_items]
    assert db.type_consensus_batch(fwd_items) == [(b, n) for b, n in single_t]
    assert single_t[-1][0] == -1 and single_t[-2] == (-1, 0)
    # the samples of a cohort repeat the common alleles: a batch scores equal consensuses once and hands every copy its result
    repeated = [items[0], items[3], items[0], items[1], items[3], items[0]]
    assert db.score_consensus_batch(repeated) == [single[k] for k in (0, 3, 0, 1, 3, 0)]
    assert db.type_consensus_batch([fwd_items[2], fwd_items[2], fwd_items[0]]) == [single_t[2], single_t[2], single_t[0]]


def test_k1_sliced_batches(oracle, pkg, gpu_ctx, small, monkeypatch, k1_exhaustive):
    """big read batches are processed in slices (shallow views of the same packed reads): identical output, slice by slice"""
    from pb_starphase_amd import synth
    fx, db = small
    rng = np.random.default_rng(13)
    reads = []
    for g in range(len(fx.genes)):
        for a in rng.choice(fx.full_length_alleles(g), 2, replace=False).tolist():
            hap, s = fx.haplotype(g, a)
            reads += synth.simulate_reads(rng, hap, s, len(fx.dna[a]), 5, mean_len=6000, sd_len=800)
    rs = gpu_ctx.upload(reads)
    whole, cells = db.realign_reads(rs, cells=True)
    monkeypatch.setenv("SP_K1_SLICE", "7")
    sliced, cells2 = db.realign_reads(rs, cells=True)
    assert sliced.tobytes() == whole.tobytes() and (cells2 == cells).all()
    assert db.realign_reads(rs).tobytes() == whole.tobytes()


def test_k1_gene_vote_filter(oracle, pkg, gpu_ctx, small, k1_exhaustive):
    """a read is only scored against the alleles of genes whose reference got >= 16 anchor votes and >= 1/10 of the best
    gene's votes.  A read of one gene leaves the other gene's cells empty; a chimeric read (an HLA-A haplotype followed by an HLA-B one) anchors in
    both and has cells in both; the cell matrix equals the oracle's in every case."""
    fx, db = small
    ga = [a for a in range(len(fx.ids)) if fx.gene_of[a] == 0 and fx.dna[a]]
    gb = [a for a in range(len(fx.ids)) if fx.gene_of[a] == 1 and fx.dna[a]]
    ha, sa = fx.haplotype(0, ga[0]); hb, sb = fx.haplotype(1, gb[0])
    read_a = ha[sa:sa + len(fx.dna[ga[0]])]
    read_b = hb[sb:sb + len(fx.dna[gb[0]])]
    chimera = read_a + read_b
    reads = [read_a, read_b, chimera]
    rs = gpu_ctx.upload(reads)
    out, cells = db.realign_reads(rs, cells=True)
    exp, ecells = hx.k1_expected(oracle, fx, reads)
    assert (cells == ecells).all(), np.argwhere(cells != ecells)[:10]
    for r, e in enumerate(exp):
        assert out[r]["status"] == e["status"] and out[r]["best_allele"] == e["best_allele"], (r, out[r], e)
    none = 0xFFFFFFFF
    in_a, in_b = np.array(fx.gene_of) == 0, np.array(fx.gene_of) == 1
    has_dna = np.array([bool(d) for d in fx.dna])
    assert (cells[0][in_b] == none).all() and (cells[0][in_a & has_dna] != none).any()
    assert (cells[1][in_a] == none).all() and (cells[1][in_b & has_dna] != none).any()
    # the chimera is anchored in both genes: cells were run in both
    assert (cells[2][in_a & has_dna] != none).any() and (cells[2][in_b & has_dna] != none).any()


K1_STAGE_NAMES = ("anchor_k1", "anchor_k1_rev", "k1_cells", "k1_cells_deep", "k1_reduce", "k1_finalize", "k1_seg_retry", "k1_seg_rescore")
# launches per profile name of ONE realign_reads call on the reads of the test below, mode by mode: what this same test body recorded with the library of the
# commit before K1's host driver was cut into stages (SP_LIB_PATH named that build)
K1_STAGE_LAUNCHES = {
    "seeded": dict(zip(K1_STAGE_NAMES, (1, 0, 0, 0, 0, 1, 1, 1))),
    "pruned": dict(zip(K1_STAGE_NAMES, (1, 1, 1, 2, 1, 1, 0, 0))),
    "cells": dict(zip(K1_STAGE_NAMES, (1, 1, 1, 0, 1, 1, 0, 0))),
}


def test_k1_modes_run_their_own_stages(pkg, gpu_ctx, small):
    """the three pipelines of sp_hla_realign_reads (seeded, pruned exhaustive, cell matrix) each record their own stages in the profile and no other mode's; and
    the exhaustive search without the affine re-score (mm2_rescore 0) gives the same records with the mm2_* fields left zero"""
    from pb_starphase_amd import synth
    fx, db = small
    rng = np.random.default_rng(17)
    reads = []
    for g in range(len(fx.genes)):
        for a in rng.choice(fx.full_length_alleles(g), 2, replace=False).tolist():
            hap, gs = fx.haplotype(g, a)
            reads += synth.simulate_reads(rng, hap, gs, len(fx.dna[a]), 6, mean_len=6500, sd_len=1200)
    reads = reads[:22]
    reads.append(synth.mutate(rng, reads[1], 20, 10, 10))           # more edits than the first pass allows
    reads.append("".join(rng.choice(list("ACGT"), 5000)))           # junk read: no allele
    s = list(reads[3])
    for p in rng.choice(len(s), 6, replace=False):
        s[int(p)] = "N"
    reads[3] = "".join(s)
    reads[5] = synth.revcomp(reads[5])
    rs = gpu_ctx.upload(reads)
    got = {}
    try:
        gpu_ctx.set_option("k1_best_n", 0)
        rescored = db.realign_reads(rs)
        gpu_ctx.set_option("mm2_rescore", 0)
        plain = db.realign_reads(rs)
        gpu_ctx.set_option("mm2_rescore", 1)
        for mode, best_n, cells in (("seeded", 5, False), ("pruned", 0, False), ("cells", 0, True)):
            gpu_ctx.set_option("k1_best_n", best_n)
            gpu_ctx.profile_reset()
            db.realign_reads(rs, cells=cells)
            got[mode] = {n: gpu_ctx.profile_get(n)[1] for n in K1_STAGE_NAMES}
    finally:
        gpu_ctx.set_option("mm2_rescore", 1)
        gpu_ctx.set_option("k1_best_n", 5)
    print("K1 stage launches:", got)
    assert (rescored["status"] == 0).sum() >= len(reads) - 4 and (rescored["mm2_score"] > 0).sum() >= len(reads) - 4
    for name in plain.dtype.names:
        if name.startswith("mm2_"):
            assert not plain[name].any(), name
        else:
            assert (plain[name] == rescored[name]).all(), name
    assert got == K1_STAGE_LAUNCHES
    for mode, mine, others in (("seeded", ("anchor_k1", "k1_finalize", "k1_seg_retry", "k1_seg_rescore"), ("k1_cells", "k1_cells_deep", "k1_reduce", "anchor_k1_rev")),
                               ("pruned", ("anchor_k1", "k1_cells", "k1_reduce", "k1_finalize"), ("k1_seg_retry", "k1_seg_rescore")),
                               ("cells", ("anchor_k1", "k1_cells", "k1_reduce", "k1_finalize"), ("k1_seg_retry", "k1_seg_rescore"))):
        assert all(got[mode][n] > 0 for n in mine) and not any(got[mode][n] for n in others), (mode, got[mode])


def test_k1_reverse_strand_reads_are_dropped(oracle, pkg, gpu_ctx, small, k1_exhaustive):
    """src/hla/realigner.rs:178-193: a read whose best mapping is on the reverse strand is dropped.  The library decides the strand at the seeds
    (status 2: the best anchor on the reverse-complemented gene references out-votes the best forward anchor); == the oracle's statement.  The
    reverse complement of a good read is dropped, the read itself is not; junk stays status 1; a read whose forward half is long enough stays."""
    from pb_starphase_amd import synth
    fx, db = small
    rng = np.random.default_rng(21)
    g = 0
    a = int(rng.choice(fx.full_length_alleles(g)))
    hap, gs = fx.haplotype(g, a)
    good = synth.simulate_reads(rng, hap, gs, len(fx.dna[a]), 4, mean_len=6500, sd_len=1000)
    reads = list(good) + [synth.revcomp(r) for r in good]
    reads.append("".join(rng.choice(list("ACGT"), 4000)))                                   # junk: neither strand
    reads.append(good[0] + synth.revcomp(good[1])[:600])                                     # a forward read with a reverse tail: stays
    reads.append(good[0][:300] + synth.revcomp(good[1]))                                     # a reverse read with a short forward head: dropped
    rs = gpu_ctx.upload(reads)
    out = db.realign_reads(rs)
    exp, _cells = hx.k1_expected(oracle, fx, reads)
    assert [int(o["status"]) for o in out] == [e["status"] for e in exp]
    assert [int(o["status"]) for o in out[:4]] == [0, 0, 0, 0] and [int(o["status"]) for o in out[4:8]] == [2, 2, 2, 2]
    assert int(out[8]["status"]) == 1 and int(out[9]["status"]) == 0 and int(out[10]["status"]) == 2
    full, _c = db.realign_reads(rs, cells=True)
    assert full.tobytes() == out.tobytes()

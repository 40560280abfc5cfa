"""sp_hla_map_ties (SP_HLA_MAP_TIES on sp_hla_map_consensus_ex / _batch_ex / sp_hla_map_type_consensus_ex): the class of every allowed allele of a consensus against
the winner of each of the two scans -- distinct, score_only, equal, beats_winner, winner (include/starphase_hip.h) -- against tests/hla_ties_ref.py, which builds
every level record from alignments and CIGARs and asks oracle/liboracle.so's osp_is_better_match both ways.

Where the reference's alignments come from:
  scan 1 (a = 5)     the map's own handed-out alignments and CIGARs (hla_ties_ref.records_from_map)
  scan 0 (unit cost) the map does not hand those out per allele: the same (allele, consensus) pairs go through Context.anchor_batch + Context.align_batch, the public
                     cell contract, and the records are built from THOSE alignments (hla_ties_ref.records_from_cells)

  1. a designed gene: copies of the consensus's allele before and behind it, an intron SNV, an exon SNV, a cDNA-only copy, a copy that overhangs the consensus
  2. fuzz, seeds 1 - 8: every allele is the consensus's allele with 0 - 3 small edits, so near-ties dominate
  3. the four configs[1] consensuses of tests/golden/concordance.json.gz against the bundled database (a = 5 scan)
  4. the batch form gives the classes and counts of the single calls, byte for byte
  5. without the flag sp_hla_map_ties fails with SP_ERR_INVALID_ARG and every other output is the flagged map's
  6. a warm context allocates nothing with ties on"""
import ctypes as C
import gzip
import json
import os
import zlib

import numpy as np
import pytest

import hla_ties_ref as ref
from test_gpu_hla_map import same_allele

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "concordance.json.gz")
NAMES = ("distinct", "score_only", "equal", "beats_winner", "winner")


def small_gene(pkg):
    from pb_starphase_amd import synth
    fx = synth.HlaFixture(genes=["HLA-A"], max_alleles_per_gene=60)
    full = fx.full_length_alleles(0)
    base = full[len(full) // 2]
    assert 0 < base < len(fx.ids) - 8
    return fx, base


def check_against_reference(gpu_ctx, fx, m, scans=(0, 1)):
    """classes and counts of map m against the reference, every allowed allele -> {scan: reference classes}"""
    out = {}
    for scan in scans:
        if scan == 1:
            recs = ref.records_from_map(m, lambda lv, a: len((fx.cdna, fx.dna)[lv][a]))
            winner = m.best_mm2
        else:
            recs = ref.records_from_cells(gpu_ctx, m.alleles, (fx.cdna, fx.dna), (m.cons_cdna, m.cons_dna))
            winner = m.best_allele
        w = list(m.alleles).index(winner) if winner >= 0 else -1
        assert ref.scan_winner(recs) == w, (scan, "the reference's own running best is not the scan's winner", ref.scan_winner(recs), w)
        cls, counts = ref.classify(recs, w)
        bad = [(int(m.alleles[k]), NAMES[m.ties[scan][k]], NAMES[cls[k]]) for k in range(len(cls)) if m.ties[scan][k] != cls[k]]
        assert not bad, (scan, bad[:10])
        assert list(m.tie_counts[scan]) == list(counts)
        assert int(m.tie_counts[scan].sum()) == (len(m.alleles) if w >= 0 else 0) and int(m.tie_counts[scan][4]) == (1 if w >= 0 else 0)
        out[scan] = cls
    return out


def intron_position(dna, cdna):
    """a DNA position whose 60-base surroundings share no 20-mer with the cDNA: inside an intron, away from the exons"""
    kmers = {cdna[i:i + 20] for i in range(len(cdna) - 19)}
    for p in range(400, len(dna) - 400):
        if not any(dna[i:i + 20] in kmers for i in range(p - 60, p + 41)):
            return p
    raise AssertionError("no intron position")


def exon_position(dna, cdna):
    """(cDNA position, DNA position) of one base in the middle of an exon: its 31-mer occurs once in the DNA"""
    for q in range(len(cdna) // 2, len(cdna) - 40):
        k = cdna[q - 15:q + 16]
        if dna.count(k) == 1:
            return q, dna.index(k) + 15
    raise AssertionError("no exon position")


def flip(s, p):
    return s[:p] + "ACGT"[("ACGT".index(s[p]) + 1) % 4] + s[p + 1:]


def test_designed_gene(pkg, gpu_ctx):
    fx, base = small_gene(pkg)
    rng = np.random.default_rng(11)
    dna, cdna = fx.dna[base], fx.cdna[base]
    earlier, later, intron, exon, cdna_only, overhang = 0, base + 1, base + 2, base + 3, base + 4, base + 5
    fx.dna[earlier], fx.cdna[earlier] = dna, cdna                               # a copy in front: the winner; base itself is then `equal`
    fx.dna[later], fx.cdna[later] = dna, cdna                                   # a copy behind
    fx.dna[intron], fx.cdna[intron] = flip(dna, intron_position(dna, cdna)), cdna
    q, p = exon_position(dna, cdna)
    fx.dna[exon], fx.cdna[exon] = flip(dna, p), flip(cdna, q)
    fx.dna[cdna_only], fx.cdna[cdna_only] = "", cdna                            # presence rule at the DNA level
    fx.dna[overhang], fx.cdna[overhang] = dna + "".join("ACGT"[x] for x in rng.integers(0, 4, 30)), cdna      # equal edits on the overlap, 30 unmapped bases
    # the classes below are what the CPU reference gave for this design (both scans), not what the kernel gave
    expected = {earlier: ref.WINNER, base: ref.EQUAL, later: ref.EQUAL, intron: ref.DISTINCT, exon: ref.DISTINCT, cdna_only: ref.DISTINCT, overhang: ref.SCORE_ONLY}
    db = fx.make_db(pkg, gpu_ctx)
    m = db.map_consensus(0, dna, cdna, ties=True)
    assert len(m.alleles) == 60 and m.best_allele == m.best_mm2 == earlier
    got = check_against_reference(gpu_ctx, fx, m)
    for scan in (0, 1):
        print("scan", scan, "counts", dict(zip(NAMES, m.tie_counts[scan].tolist())), "designed", {a: NAMES[got[scan][list(m.alleles).index(a)]] for a in expected})
        for a, want in expected.items():
            assert m.ties[scan][list(m.alleles).index(a)] == got[scan][list(m.alleles).index(a)] == want, (scan, a, NAMES[want])
    # cDNA scoring disabled (DNA is then required): the cDNA-only copy is not scored at all; the rest is classified on the DNA level alone
    m2 = db.map_consensus(0, dna, cdna, require_dna=True, disable_cdna=True, ties=True)
    assert cdna_only not in list(m2.alleles) and all(fx.dna[a] for a in m2.alleles)
    got2 = check_against_reference(gpu_ctx, fx, m2)
    for scan in (0, 1):
        for a, want in expected.items():
            if a != cdna_only:
                assert got2[scan][list(m2.alleles).index(a)] == want, (scan, a, NAMES[want])


def fuzz_edit(rng, s):
    for _ in range(int(rng.integers(0, 4))):
        kind = int(rng.integers(0, 4))
        p = int(rng.integers(20, len(s) - 20))
        if kind == 0:
            s = flip(s, p)
        elif kind == 1:
            s = s[:p] + s[p + int(rng.integers(1, 4)):]
        elif kind == 2:
            s = s[:p] + "".join("ACGT"[x] for x in rng.integers(0, 4, int(rng.integers(1, 4)))) + s[p:]
        else:
            cut = int(rng.integers(0, 201))
            s = s[cut:] if rng.random() < 0.5 else s[:len(s) - cut]
    return s


@pytest.mark.parametrize("seed", range(1, 9))
def test_fuzz(pkg, gpu_ctx, seed):
    fx, base = small_gene(pkg)
    rng = np.random.default_rng(seed)
    dna, cdna = fx.dna[base], fx.cdna[base]
    for a in range(len(fx.ids)):
        fx.dna[a], fx.cdna[a] = fuzz_edit(rng, dna), fuzz_edit(rng, cdna)
    m = fx.make_db(pkg, gpu_ctx).map_consensus(0, dna, cdna, ties=True)
    got = check_against_reference(gpu_ctx, fx, m)
    for scan in (0, 1):
        print("seed", seed, "scan", scan, dict(zip(NAMES, np.bincount(got[scan], minlength=5).tolist())), "beats_winner cases met:", int((got[scan] == ref.BEATS_WINNER).sum()))


@pytest.fixture(scope="module")
def hla(pkg, gpu_ctx):
    from pb_starphase_amd import synth
    fx = synth.HlaFixture()
    return fx, fx.make_db(pkg, gpu_ctx)


@pytest.fixture(scope="module")
def maps(hla):
    fx, db = hla
    with gzip.open(GOLDEN, "rt") as f:
        gold = json.load(f)
    out = []
    for row in gold["k2"]["consensuses"]:
        gi = fx.genes.index(row["gene"])
        cons = [c for c in gold["hla"]["consensus"][row["gene"]] if zlib.crc32(c.encode()) & 0xFFFFFFFF == row["consensus_crc"]][0]
        out.append((gi, cons, db.map_type_consensus(gi, cons, ties=True)))
    assert len(out) == 4
    return out


def test_the_four_consensuses_of_the_bundled_database(gpu_ctx, hla, maps):
    fx, _db = hla
    for gi, _cons, m in maps:
        cls = check_against_reference(gpu_ctx, fx, m, scans=(1,))[1]
        w = m.best_mm2
        assert w >= 0
        same = [k for k, x in enumerate(m.alleles) if same_allele(fx, w, int(x))]
        assert all(cls[k] in (ref.EQUAL, ref.WINNER) for k in same) and all(m.ties[1][k] in (ref.EQUAL, ref.WINNER) for k in same)
        print(fx.genes[gi], "alleles", len(m.alleles), "mm2", dict(zip(NAMES, m.tie_counts[1].tolist())), "unit", dict(zip(NAMES, m.tie_counts[0].tolist())), "same sequences as the winner", len(same))


def test_batch_equals_single_calls(hla, maps):
    _fx, db = hla
    items = [(gi, m.cons_dna, m.cons_cdna) for gi, _cons, m in maps]
    batch = db.map_consensus_batch(items, ties=True)
    assert len(batch) == 4
    for (gi, _cons, m), it, b in zip(maps, items, batch):
        s = db.map_consensus(*it, ties=True)
        for scan in (0, 1):
            assert s.ties[scan].tobytes() == b.ties[scan].tobytes() == m.ties[scan].tobytes()
            assert s.tie_counts[scan].tobytes() == b.tie_counts[scan].tobytes() == m.tie_counts[scan].tobytes()


def same_map(x, m):
    return (x.gene == m.gene and x.best_allele == m.best_allele and x.best_mm2 == m.best_mm2 and np.array_equal(x.alleles, m.alleles) and np.array_equal(x.stats_mm2, m.stats_mm2)
            and np.array_equal(x.aln, m.aln) and np.array_equal(x.diag, m.diag) and x.cons_cdna == m.cons_cdna and x.cons_dna == m.cons_dna
            and all(np.array_equal(x.cigar[lv][k], m.cigar[lv][k]) for lv in (0, 1) for k in range(len(m.alleles))))


def test_without_the_flag_there_are_no_ties_and_nothing_else_changes(pkg, gpu_ctx, hla, maps):
    _fx, db = hla
    L = pkg.ffi.lib()
    gi, cons, m = maps[0]
    for make in (lambda h: L.sp_hla_map_consensus(gpu_ctx._h, db._h, gi, m.cons_dna.encode(), len(m.cons_dna), m.cons_cdna.encode(), len(m.cons_cdna), 0, 0, C.byref(h)),
                 lambda h: L.sp_hla_map_consensus_ex(gpu_ctx._h, db._h, gi, m.cons_dna.encode(), len(m.cons_dna), m.cons_cdna.encode(), len(m.cons_cdna), 0, 0, 0, C.byref(h)),
                 lambda h: L.sp_hla_map_type_consensus(gpu_ctx._h, db._h, gi, cons.encode(), len(cons), 0, 0, C.byref(h)),
                 lambda h: L.sp_hla_map_type_consensus_ex(gpu_ctx._h, db._h, gi, cons.encode(), len(cons), 0, 0, 0, C.byref(h))):
        h = C.c_void_p()
        assert make(h) == pkg.ffi.SP_OK
        p, cnt = C.c_void_p(), (C.c_uint32 * 5)()
        try:
            assert L.sp_hla_map_ties(h, 0, 1, C.byref(p), C.byref(cnt)) == pkg.ffi.SP_ERR_INVALID_ARG
            assert b"SP_HLA_MAP_TIES" in L.sp_hla_map_last_error(h)
        finally:
            plain = db._read_map(h)                       # (frees the handle)
        assert len(plain) == 1 and plain[0].ties is None and same_map(plain[0], m)
    for plain, (_gi, _cons, mm) in zip(db.map_consensus_batch([(g, x.cons_dna, x.cons_cdna) for g, _c, x in maps]), maps):
        assert same_map(plain, mm)
    h = C.c_void_p()
    assert L.sp_hla_map_type_consensus_ex(gpu_ctx._h, db._h, gi, cons.encode(), len(cons), 0, 0, 2, C.byref(h)) == pkg.ffi.SP_ERR_INVALID_ARG and not h.value     # an unknown flag


def test_a_warm_context_allocates_nothing_with_ties_on(gpu_ctx, hla, maps):
    """sp_profile_get("pool:device") counts every device allocation of the context's pooled buffers (the class bytes and the counts are two of them); the library keeps no
    counter of host allocations, so the device pool is what is asserted, as tests/test_gpu_hla_map.py does"""
    _fx, db = hla
    items = [(gi, m.cons_dna, m.cons_cdna) for gi, _cons, m in maps]
    db.map_consensus_batch(items, ties=True)
    _ms, allocs0, bytes0 = gpu_ctx.profile_get("pool:device")
    launches0 = gpu_ctx.profile_get("k2_ties")[1]
    db.map_consensus_batch(items, ties=True)
    _ms, allocs1, bytes1 = gpu_ctx.profile_get("pool:device")
    assert allocs0 > 0 and allocs1 == allocs0 and bytes1 == bytes0
    assert gpu_ctx.profile_get("k2_ties")[1] == launches0 + 1
    db.map_consensus_batch(items)                          # and without the flag: no launch of the pass
    assert gpu_ctx.profile_get("k2_ties")[1] == launches0 + 1 and gpu_ctx.profile_get("pool:device")[1:] == (allocs1, bytes1)

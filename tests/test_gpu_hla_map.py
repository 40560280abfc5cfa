"""sp_hla_map_consensus(_batch) / sp_hla_map_type_consensus: score_read's per-allele mappings (src/hla/caller.rs:1332-1511) -- for every (consensus, level, allowed allele)
the two-piece affine alignment at a = 5 on the 64 diagonals around the diagonal K2's own cell found, with its CIGAR, from a traceback that keeps checkpoints and an LDS
tile instead of a direction byte per cell (sp_affine.hip: affine_map_kernel).

  1. bit-identical to sp_affine_align_batch (band 64, same scores) on the pairs rebuilt from the map's own diagonals: every pair of the four configs[1] consensuses at
     both levels, and a synthetic gene with 40 - 100-base indels and N bases
  2. the ops spell out score, NM and spans (tests/affine_traceback_ref.py: check_ops) on 200 sampled pairs
  3. the winner's rows of stats_mm2 are sp_hla_best.mm2_stats of sp_hla_type_consensus
  4. stats_mm2 against the reference-call-pattern port's numbers (tests/golden/concordance.json.gz, k2): measured, not below the unit-cost share of the same test,
     and not below the floor measured when this test was written; best_mm2 names the port's winner on 4 of 4
  5. the batch form gives what the single calls give
  6. a warm context makes no device allocation: asserted through the context's pool statistics (sp_profile_get "pool:device")"""
import gzip
import json
import os
import zlib

import numpy as np
import pytest

import affine_traceback_ref as tb

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "concordance.json.gz")
# the share of (allele, level) pairs of the four configs[1] consensuses whose (nm, unmapped) from stats_mm2 equal the port's, mapped-by-either as the denominator:
# the value measured on MI355X, rounded down to three decimals (profiles/hla_map/k2_numbers.txt)
K2_MM2_SAME_FLOOR = 0.999


@pytest.fixture(scope="module")
def gold():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def hla(pkg, gpu_ctx):
    from pb_starphase_amd import synth
    fx = synth.HlaFixture()
    return fx, fx.make_db(pkg, gpu_ctx)


def same_allele(fx, a, b):
    return a == b or (a >= 0 and b >= 0 and fx.cdna[a] == fx.cdna[b] and fx.dna[a] == fx.dna[b])


def consensuses(fx, gold):
    out = []
    for row in gold["k2"]["consensuses"]:
        gi = fx.genes.index(row["gene"])
        cons = [c for c in gold["hla"]["consensus"][row["gene"]] if zlib.crc32(c.encode()) & 0xFFFFFFFF == row["consensus_crc"]][0]
        out.append((row, gi, cons))
    assert len(out) == 4
    return out


@pytest.fixture(scope="module")
def maps(hla, gold):
    fx, db = hla
    return [(row, gi, cons, db.map_type_consensus(gi, cons)) for row, gi, cons in consensuses(fx, gold)]


def check_against_align_batch(ctx, m, seqs_of_level, stride=2048):
    """every mapping of HlaMap m against sp_affine_align_batch on the pair rebuilt from the map's diagonal -> number of pairs compared.  A pair without a mapping has
    score 0 and no ops; it is compared too when the allele has a sequence at that level (max_ed < 0 is not used: the pair runs on diagonal 0 only when the map has none)."""
    n_cmp = 0
    for lv in (0, 1):
        target = m.cons_cdna if lv == 0 else m.cons_dna
        mapped = [k for k in range(len(m.alleles)) if m.aln[lv, k]["score"] > 0]
        is_mapped = set(mapped)
        for k in range(len(m.alleles)):
            if k not in is_mapped:
                assert len(m.cigar[lv][k]) == 0 and tuple(m.stats_mm2[k, 3 * lv:3 * lv + 3]) == (-1, -1, -1)
        if not mapped:
            continue
        A = ctx.upload([seqs_of_level[lv][int(m.alleles[k])] for k in mapped])
        B = ctx.upload([target])
        out, cigar, n_cigar = ctx.affine_align(A, B, [(x, 0, int(m.diag[lv, k])) for x, k in enumerate(mapped)], a=5, band=64, cigar_stride=stride)
        for x, k in enumerate(mapped):
            assert out[x] == m.aln[lv, k], (lv, k, out[x], m.aln[lv, k])
            assert int(n_cigar[x]) == len(m.cigar[lv][k]) <= stride, (lv, k)
            assert np.array_equal(cigar[x, :n_cigar[x]], m.cigar[lv][k]), (lv, k)
            n_cmp += 1
    return n_cmp


def test_map_is_bit_identical_to_the_existing_traceback(gpu_ctx, hla, maps):
    fx, _db = hla
    total = 0
    for row, gi, cons, m in maps:
        assert m is not None and list(m.alleles) == [a for a in range(len(fx.ids)) if fx.gene_of[a] == gi]
        n = check_against_align_batch(gpu_ctx, m, (fx.cdna, fx.dna))
        mapped = int((m.aln["score"] > 0).sum())
        assert n == mapped > 0
        total += n
        print(row["gene"], "alleles", len(m.alleles), "mapped (allele, level) pairs compared", n)
    print("pairs compared:", total)


def test_map_on_a_synthetic_gene_with_long_indels_and_n(pkg, gpu_ctx):
    """alleles with a 40 - 100-base insertion or deletion against the consensus (the second gap piece, 26 + l, and paths near the band's edge) and alleles with N bases"""
    from pb_starphase_amd import synth
    fx = synth.HlaFixture(genes=["HLA-A"], max_alleles_per_gene=60)
    rng = np.random.default_rng(77)
    full = fx.full_length_alleles(0)
    base = full[0]
    cons_dna, cons_cdna = fx.dna[base], fx.cdna[base]
    changed = 0
    for a in full[1:]:
        s = fx.dna[a]
        kind = changed % 3
        pos = int(rng.integers(300, len(s) - 300)); ln = int(rng.integers(40, 101))
        if kind == 0:
            s = s[:pos] + s[pos + ln:]
        elif kind == 1:
            s = s[:pos] + "".join("ACGT"[x] for x in rng.integers(0, 4, ln)) + s[pos:]
        else:
            b = list(s)
            for p in rng.integers(50, len(s) - 50, 12):
                b[int(p)] = "N"
            s = "".join(b)
            c = list(fx.cdna[a]); c[len(c) // 2] = "N"; fx.cdna[a] = "".join(c)
        fx.dna[a] = s
        changed += 1
    assert changed >= 6
    db = fx.make_db(pkg, gpu_ctx)
    m = db.map_consensus(0, cons_dna, cons_cdna)
    n = check_against_align_batch(gpu_ctx, m, (fx.cdna, fx.dna))
    long_gaps = sum(1 for k in range(len(m.alleles)) for w in m.cigar[1][k] if (int(w) & 15) in (1, 2) and (int(w) >> 4) >= 40)
    print("synthetic gene: pairs compared", n, "gap runs of 40 bases or more", long_gaps)
    assert n >= len(full) and long_gaps >= 2


def test_ops_spell_out_score_nm_and_spans(hla, maps):
    fx, _db = hla
    rng = np.random.default_rng(5)
    cand = [(ci, lv, k) for ci, (_r, _g, _c, m) in enumerate(maps) for lv in (0, 1) for k in range(len(m.alleles)) if m.aln[lv, k]["score"] > 0]
    picks = [cand[i] for i in rng.choice(len(cand), 200, replace=False)]
    for ci, lv, k in picks:
        m = maps[ci][3]
        al = m.aln[lv, k]
        target = m.cons_cdna if lv == 0 else m.cons_dna
        query = (fx.cdna if lv == 0 else fx.dna)[int(m.alleles[k])]
        ops = tb.decode_ops(m.cigar[lv][k], len(m.cigar[lv][k]))
        nm, score = tb.check_ops(ops, target, query, int(al["b_start"]), int(al["b_end"]), int(al["a_start"]), int(al["a_end"]), a=5)
        assert (nm, score) == (int(al["nm"]), int(al["score"])), (ci, lv, k, nm, score, al)


def test_winner_rows_are_mm2_stats(hla, maps):
    fx, db = hla
    for row, gi, cons, m in maps:
        best, _n, _st, _cdna = db.type_consensus(gi, cons, stats=False)
        assert int(best) == m.best_allele >= 0
        k = list(m.alleles).index(int(best))
        assert list(m.stats_mm2[k]) == list(db.last_mm2_stats), (row["gene"], list(m.stats_mm2[k]), db.last_mm2_stats)


def test_numbers_against_the_port(hla, maps):
    """the share of (allele, level) pairs with the port's (nm, unmapped): stats_mm2 against the unit-cost rows of sp_hla_type_consensus, counted as
    tests/test_gpu_concordance.py counts (mapped by either is the denominator)"""
    fx, db = hla
    same_mm2 = same_unit = all_mm2 = all_unit = winners = 0
    for row, gi, cons, m in maps:
        port = np.array(row["nm_unmapped"], np.int64)
        idx = [int(a) for a in m.alleles]
        assert len(idx) == row["n_alleles"] and idx[0] == row["first_allele"]
        _best, _n, st, _cdna = db.type_consensus(gi, cons, stats=True)
        unit = st[idx].astype(np.int64)
        mm2 = m.stats_mm2.astype(np.int64)
        for lv, (cn, cu) in enumerate(((1, 2), (4, 5))):
            p_nm, p_un = port[:, 2 * lv], port[:, 2 * lv + 1]
            for which, rows in (("mm2", mm2), ("unit", unit)):
                l_nm, l_un = rows[:, cn], rows[:, cu]
                either = int(((p_nm >= 0) | (l_nm >= 0)).sum())
                same = int(((p_nm >= 0) & (l_nm >= 0) & (p_nm == l_nm) & (p_un == l_un)).sum())
                if which == "mm2":
                    all_mm2 += either; same_mm2 += same
                else:
                    all_unit += either; same_unit += same
        winners += same_allele(fx, m.best_mm2, row["winner"])
        print(row["gene"], "best_allele", m.best_allele, "best_mm2", m.best_mm2, "port", row["winner"])
    share_mm2, share_unit = same_mm2 / max(1, all_mm2), same_unit / max(1, all_unit)
    print("K2 (allele, level) pairs with the port's (nm, unmapped): stats_mm2 %d of %d = %.4f ; unit-cost %d of %d = %.4f" % (same_mm2, all_mm2, share_mm2, same_unit, all_unit, share_unit))
    assert winners == 4
    assert share_mm2 >= share_unit
    assert share_mm2 >= K2_MM2_SAME_FLOOR


def test_batch_equals_single_calls(hla, maps):
    fx, db = hla
    singles = [db.map_consensus(gi, m.cons_dna, m.cons_cdna) for _row, gi, _cons, m in maps]
    batch = db.map_consensus_batch([(gi, m.cons_dna, m.cons_cdna) for _row, gi, _cons, m in maps])
    assert len(batch) == 4
    for (_row, _gi, _cons, m), s, b in zip(maps, singles, batch):
        for x in (s, b):
            assert x.gene == m.gene and x.best_allele == m.best_allele and x.best_mm2 == m.best_mm2
            assert np.array_equal(x.alleles, m.alleles) and np.array_equal(x.stats_mm2, m.stats_mm2)
            assert np.array_equal(x.aln, m.aln) and np.array_equal(x.diag, m.diag)
            assert all(np.array_equal(x.cigar[lv][k], m.cigar[lv][k]) for lv in (0, 1) for k in range(len(m.alleles)))


def test_a_warm_context_allocates_nothing(gpu_ctx, hla, maps):
    """relies on the context's pool statistics: sp_profile_get("pool:device") counts every device allocation of the context's pooled buffers and its scratch.  That is what
    the map path allocates from (k2_score_batch and sp_launch_affine_map take every buffer from sp_pool, the consensus set from sp_seqset_make_small, which is pooled too);
    memory a sequence set or a database owns is not counted, and the map path makes none."""
    fx, db = hla
    items = [(gi, m.cons_dna, m.cons_cdna) for _row, gi, _cons, m in maps]
    db.map_consensus_batch(items)
    _ms, allocs0, bytes0 = gpu_ctx.profile_get("pool:device")
    db.map_consensus_batch(items)
    _ms, allocs1, bytes1 = gpu_ctx.profile_get("pool:device")
    print("pooled device memory: allocations", allocs0, "->", allocs1, "bytes", bytes0, "->", bytes1)
    assert allocs0 > 0 and allocs1 == allocs0 and bytes1 == bytes0

"""update-hla on the device: sp_hla_config_extend (HlaConfig::new, src/hla/alleles.rs:109-207, as one batch of (allele, strand) cells per gene: anchor, two-piece
affine re-score, hlacfg_pick_extend_kernel) against the minimap2 restatement, and the `starphase_hip update-hla` command end to end.  The shapes are the
smallest that reach every branch: two genes on the two chr6 islands, at most 18 alleles of about 3.5 kb, batches of 1, 3 and 16 alleles (one, several and
fewer than one wave of picks per fold)."""
import json
import subprocess

import pytest

import hla_update_cases as hc
import test_oracle_mm2 as tm

pytestmark = pytest.mark.gpu
FIELDS = ("rev", "nm", "q_start", "q_end", "t_start", "t_end")


@pytest.fixture(scope="module")
def mm():
    return tm.mm2_ffi.Mm2()


@pytest.fixture(scope="module")
def world(pkg, tmp_path_factory):
    """the chr6 reference, the database with the RefSeq records and the designed set, made once"""
    tmp = tmp_path_factory.mktemp("hla_update")
    D = pkg.database
    db_path = tmp / "refseq_db.json"
    db_path.write_text(json.dumps(hc.refseq_database(variant_db="CACNA1S")))
    return dict(tmp=tmp, D=D, chr6=hc.write_chr6(tmp / "chr6.fa"), db_path=str(db_path))


@pytest.fixture(scope="module")
def designed(mm):
    S = hc.designed_set(mm)
    ids = {a[2]: "HLA:HLA9%04d" % i for i, a in enumerate(S)}
    return S, hc.oracle_extend(mm, S, ids)                  # the oracle side, computed once


def run(world, gpu_ctx, gen, nuc, batch=0, db=True):
    """-> ({star description: record or None}, {gene: (start, end, moved, worst description, worst stats)}, result)"""
    D = world["D"]
    A = D.HlaAlleles.load(gen, nuc)
    R = gpu_ctx.hla_config_extend(D.Fasta(world["chr6"]), A, D.Database(world["db_path"]) if db else None, batch_alleles=batch)
    alleles = [A.allele(i) for i in range(len(A))]
    desc = [a["gene_name"][4:] + "*" + ":".join(a["star_allele"]) for a in alleles]
    maps = R.mappings()
    assert R.overflow == [] and R.warnings == ""
    genes = {g["name"]: (g["start"], g["end"], g["moved"], None if g["worst_allele"] is None else desc[g["worst_allele"]], g["worst"]) for g in R.genes()}
    return dict(zip(desc, maps)), genes, R


def test_the_reference_pin(world, gpu_ctx, mm):
    """test_hlaconfig_new (src/hla/alleles.rs:512-547): the two real alleles against the RefSeq records +- 2,000 bases end at HlaConfig::default()'s coordinates"""
    recs, genes, R = run(world, gpu_ctx, hc.FAUX_GEN, hc.FAUX_NUC)
    for name, _s, _e, want in tm.HLACONFIG_CASES:
        assert genes["HLA-" + name[0]][:3] == (want[0], want[1], True), (name, genes)
    a, b = recs["A*01:01:01:01"], recs["B*07:02:01:01"]
    assert (a["rev"], a["nm"]) == (0, 42) and (b["rev"], b["nm"]) == (1, 0)
    # the mappings of the minimap2 restatement (what the per-allele Python loop of tests/test_gpu_hlaconfig.py is held to as well), field by field
    ref = tm.hlaconfig_extend(lambda t, q: mm.map_pair(t, q), tm._islands(), tm._faux_alleles())
    for name in ("A*01:01:01:01", "B*07:02:01:01"):
        assert recs[name] == {k: int(ref[name][2][k]) for k in FIELDS}, (name, recs[name], ref[name][2])
    assert genes["HLA-A"][3:] == ("A*01:01:01:01", (3503, 42, 0)) and genes["HLA-B"][3:] == ("B*07:02:01:01", (4081, 0, 0))
    assert [(g["n_dna_alleles"], g["n_mapped"], g["is_absent_capable"]) for g in R.genes()] == [(1, 1, False), (1, 1, False)]


def test_designed_set_equals_the_oracle(world, gpu_ctx, designed):
    S, (want_recs, want_genes) = designed
    gen, nuc, _ids = hc.write_set(world["tmp"], S, tag="designed")
    recs, genes, _R = run(world, gpu_ctx, gen, nuc)
    for _g, kind, desc, _dna, _c in S:
        print(kind, desc, recs[desc], want_recs[desc])
    wrong = [(kind, desc, recs[desc], want_recs[desc]) for _g, kind, desc, _dna, _c in S if recs[desc] != want_recs[desc]]
    assert wrong == []
    assert genes == want_genes


def test_order_batch_and_tie_independence(world, gpu_ctx, mm, designed):
    S, (want_recs, want_genes) = designed
    # the ids handed out in another order: the alleles are visited in another order, nothing else may change
    order = [(7 * p + 3) % len(S) for p in range(len(S))]
    gen, nuc, ids = hc.write_set(world["tmp"], S, order=order, tag="permuted")
    assert sorted(ids.values()) != [ids[a[2]] for a in S]
    recs, genes, _R = run(world, gpu_ctx, gen, nuc)
    assert recs == want_recs and genes == want_genes
    # batches of 1, 3 and 16 alleles per pass
    gen, nuc, _ids = hc.write_set(world["tmp"], S, tag="batches")
    for batch in (1, 3, 16):
        recs, genes, _R = run(world, gpu_ctx, gen, nuc, batch=batch)
        assert recs == want_recs and genes == want_genes, batch
    # two identical alleles tie for "worst": the lower id is named, wherever the batches are cut
    twins = list(S)
    for gene, worst in (("HLA-A", "A*94:01:01:01"), ("HLA-B", "B*94:01:01:01")):
        src = next(a for a in S if a[2] == worst)
        twins.insert(0, (gene, "twin", worst.replace("*94", "*89"), src[3], src[4]))          # first in the list, LAST in id order below
    order = list(range(2, len(twins))) + [0, 1]
    gen, nuc, ids = hc.write_set(world["tmp"], twins, order=order, tag="twins")
    assert ids["A*89:01:01:01"] > ids["A*94:01:01:01"]
    for batch in (0, 1, 3):
        recs, genes, _R = run(world, gpu_ctx, gen, nuc, batch=batch)
        assert recs["A*89:01:01:01"] == recs["A*94:01:01:01"] == want_recs["A*94:01:01:01"]
        assert genes == want_genes, batch                                                       # the worst slot still names *94, the lower id


def test_gene_without_dna_and_window_off_the_chromosome(world, gpu_ctx, pkg):
    D, tmp = world["D"], world["tmp"]
    gen, nuc = hc.read_fasta(hc.FAUX_GEN), hc.read_fasta(hc.FAUX_NUC)
    # HLA-B's allele has cDNA only: the gene keeps its coordinates
    g = hc.write_fasta(tmp / "a_only_gen.fa", [(k, d, s) for k, (d, s) in gen.items() if d.startswith("A*")])
    recs, genes, R = run(world, gpu_ctx, g, hc.FAUX_NUC)
    (s, e), _want = hc.REFSEQ["HLA-B"]
    assert genes["HLA-B"] == (s, e, False, None, None) and recs["B*07:02:01:01"] is None and R.genes()[1]["n_dna_alleles"] == 0
    assert genes["HLA-A"][:3] == (29942253, 29945870, True)
    # without a database the start is HlaConfig::default(): already wide enough, nothing moves
    recs, genes, _R = run(world, gpu_ctx, hc.FAUX_GEN, hc.FAUX_NUC, db=False)
    assert [genes[k][:3] for k in ("HLA-A", "HLA-B")] == [(29942253, 29945870, False), (31353361, 31357442, False)] and recs["A*01:01:01:01"]["nm"] == 42
    # a gene at position 500 of a toy contig: its window would start before the contig
    toy = hc.refseq_database(extra_genes=[hc.gene_definition("HLA-C", "toy", 500, 3000, True, [(600, 700)])])
    (tmp / "toy_db.json").write_text(json.dumps(toy))
    fa = tmp / "toy.fa"
    fa.write_text(open(world["chr6"]).read() + ">toy\n" + "ACGT" * 2000 + "\n")
    A = D.HlaAlleles.load(hc.FAUX_GEN, hc.FAUX_NUC)
    with pytest.raises(pkg.StarphaseError) as err:
        gpu_ctx.hla_config_extend(D.Fasta(fa), A, D.Database(tmp / "toy_db.json"))
    assert err.value.code == 1 and "HLA-C" in str(err.value) and "starts before toy" in str(err.value)


def test_update_hla_command_end_to_end(world, gpu_ctx, pkg, oracle):
    D, tmp = world["D"], world["tmp"]
    out = tmp / "updated.json.gz"
    cmd = [D.cli_path(), "update-hla", "-d", world["db_path"], "-r", world["chr6"], "--hla-gen", hc.FAUX_GEN, "--hla-nuc", hc.FAUX_NUC, "--hla-version", "3.58.0", "-o", str(out), "-v"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert "HLA-A chr6:29942253-29945870 (updated)" in p.stderr and "worst mapping HLA:HLA00001 (42+0)/3503" in p.stderr
    db = D.Database(out)                                                                   # the output loads
    assert db.metadata["hla_version"] == "3.58.0" and db.stats.n_gene_entries == 1
    assert [(g["name"], g["start"], g["end"]) for g in db.hla_genes()] == [("HLA-" + n[0], w[0], w[1]) for n, _s, _e, w in tm.HLACONFIG_CASES]
    import gzip
    got = json.load(gzip.open(out))
    assert got["hla_sequences"] == D.HlaAlleles.load(hc.FAUX_GEN, hc.FAUX_NUC).table()
    assert got["gene_entries"] == json.load(open(world["db_path"]))["gene_entries"]
    # sp_hla_db_create on it, and the unchanged HLA-A allele typed as a consensus names itself with (len, 0, 0)
    isl = tm._islands()
    refs = []
    for g in db.hla_genes():
        (i0, _i1), seq = next((k, v) for k, v in isl.items() if k[0] <= g["start"] - 100 and g["end"] + 100 <= k[1])
        refs.append(seq[g["start"] - 100 - i0:g["end"] + 100 - i0])
    hdb, alleles = db.hla_db(gpu_ctx, refs)
    a = got["hla_sequences"]["HLA:HLA00001"]
    best, n_scored, stats, _cdna = hdb.type_consensus(0, a["dna_sequence"])
    print(best, n_scored, stats[best].tolist() if best >= 0 else None)
    assert alleles[best] == ("HLA:HLA00001", "HLA-A", "01:01:01:01")
    assert stats[best].tolist() == [len(a["cdna_sequence"]), 0, 0, len(a["dna_sequence"]), 0, 0]
    hdb.close()
    # a missing --hla-nuc file: NOINPUT, before any device work
    cmd[cmd.index("--hla-nuc") + 1] = str(tmp / "no_such.fa")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=60)
    assert p.returncode == 66 and "does not exist" in p.stderr
    # a FASTA error: DATAERR
    bad = hc.write_fasta(tmp / "bad_nuc.fa", [("HLA:HLA00001", "A*01:01:01:02", "ACGT")])
    cmd[cmd.index("--hla-nuc") + 1] = bad
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=60)
    assert p.returncode == 65 and "has description" in p.stderr

"""update-hla on the host: the FASTA intake (sp_hla_fasta_load: convert_fasta_str_to_map + collapse_hla_lookup, src/build_database.rs:233-325;
HlaAlleleDefinition::new, src/hla/alleles.rs:353-382) and the database writer (sp_database_save_hla).  No device.

The fixture pair tests/golden/HLA-faux/hla_gen.fa + hla_nuc.fa is the reference's test_data/HLA-faux: HLA:HLA00001 (A*01:01:01:01) and HLA:HLA00132 (B*07:02:01:01).
tests/golden/hla_faux_database.json shares the HLA-B allele with them; its HLA-A allele is another one (HLA:HLA00037, A*03:01:01:01), so the table is held to
the database for HLA-B and to the files' own content for HLA-A."""
import gzip
import json
import os
import shutil

import pytest

import hla_update_cases as hc


@pytest.fixture(scope="module")
def D(pkg):
    return pkg.database


@pytest.fixture(scope="module")
def faux():
    return hc.read_fasta(hc.FAUX_GEN), hc.read_fasta(hc.FAUX_NUC)


def records(fa):
    return [(k, d, s) for k, (d, s) in fa.items()]


def test_the_faux_files_give_their_two_alleles_in_id_order(D, faux):
    gen, nuc = faux
    A = D.HlaAlleles.load(hc.FAUX_GEN, hc.FAUX_NUC)
    assert A.stats == dict(n_alleles=2, n_dna=2, n_dropped_no_cdna=0, n_dropped_gene=0, warnings="")
    a, b = A.allele(0), A.allele(1)
    assert a == dict(hla_id="HLA:HLA00001", gene_name="HLA-A", star_allele=["01", "01", "01", "01"], dna_sequence=gen["HLA:HLA00001"][1], cdna_sequence=nuc["HLA:HLA00001"][1])
    assert (len(a["dna_sequence"]), len(a["cdna_sequence"])) == (3503, 1098)
    want = json.load(open(os.path.join(hc.GOLDEN, "hla_faux_database.json")))["hla_sequences"]["HLA:HLA00132"]
    assert b == want
    assert list(A.table()) == ["HLA:HLA00001", "HLA:HLA00132"]


def test_gzip_files_give_the_same_table(D, tmp_path):
    for name in ("hla_gen.fa", "hla_nuc.fa"):
        with open(os.path.join(hc.GOLDEN, "HLA-faux", name), "rb") as src, gzip.open(tmp_path / (name + ".gz"), "wb") as dst:
            shutil.copyfileobj(src, dst)
    assert D.HlaAlleles.load(tmp_path / "hla_gen.fa.gz", tmp_path / "hla_nuc.fa.gz").table() == D.HlaAlleles.load(hc.FAUX_GEN, hc.FAUX_NUC).table()


def test_duplicate_records(D, pkg, faux, tmp_path):
    gen, nuc = records(faux[0]), records(faux[1])
    g = hc.write_fasta(tmp_path / "gen.fa", gen + [gen[0]])                    # the same record twice: accepted
    n = hc.write_fasta(tmp_path / "nuc.fa", nuc + [nuc[1]])
    assert D.HlaAlleles.load(g, n).table() == D.HlaAlleles.load(hc.FAUX_GEN, hc.FAUX_NUC).table()
    rid, desc, seq = gen[0]
    changed = seq[:100] + ("A" if seq[100] != "A" else "C") + seq[101:]
    g = hc.write_fasta(tmp_path / "gen2.fa", gen + [(rid, desc, changed)])
    with pytest.raises(pkg.StarphaseError, match="FASTA record with multiple IDs/sequences detected: HLA:HLA00001"):
        D.HlaAlleles.load(g, n)
    g = hc.write_fasta(tmp_path / "gen3.fa", gen + [(rid, "A*01:01:01:02", seq)])   # the same sequence under another star allele is no duplicate either
    with pytest.raises(pkg.StarphaseError, match="FASTA record with multiple IDs/sequences detected: HLA:HLA00001"):
        D.HlaAlleles.load(g, n)


def test_dna_without_cdna_is_dropped_and_counted(D, faux, tmp_path):
    gen, nuc = records(faux[0]), records(faux[1])
    g = hc.write_fasta(tmp_path / "gen.fa", gen + [("HLA:HLA77777", "A*02:01:01:01", "ACGT" * 50), ("HLA:HLA77778", "B*08:01:01:01", "TTGCA" * 30)])
    A = D.HlaAlleles.load(g, hc.write_fasta(tmp_path / "nuc.fa", nuc))
    assert A.stats["n_alleles"] == 2 and A.stats["n_dropped_no_cdna"] == 2
    assert A.stats["warnings"] == "Detected 2 DNA entries that do not have a cDNA, ignoring them.\n"
    assert list(A.table()) == ["HLA:HLA00001", "HLA:HLA00132"]
    # the other way round is an allele without DNA
    A = D.HlaAlleles.load(hc.write_fasta(tmp_path / "gen1.fa", gen[:1]), hc.FAUX_NUC)
    assert A.stats["n_dna"] == 1 and A.allele(1)["dna_sequence"] is None and A.allele(1)["cdna_sequence"] == nuc[1][2]


def test_description_mismatch_is_the_reference_error(D, pkg, faux, tmp_path):
    gen, nuc = records(faux[0]), records(faux[1])
    n = hc.write_fasta(tmp_path / "nuc.fa", [(nuc[0][0], "A*01:01:01:02", nuc[0][2]), nuc[1]])
    with pytest.raises(pkg.StarphaseError) as e:
        D.HlaAlleles.load(hc.FAUX_GEN, n)
    assert 'HLA:HLA00001 has description "A*01:01:01:01" for DNA and "A*01:01:01:02" for cDNA.' in str(e.value)


def test_unsupported_gene_is_dropped_and_counted(D, faux, tmp_path):
    gen, nuc = records(faux[0]), records(faux[1])
    g = hc.write_fasta(tmp_path / "gen.fa", gen + [("HLA:HLA16001", "DPB2*01:01:01:01", "ACGT" * 50), ("HLA:HLA20000", "DRB3*01:01:02:01", "ACGGT" * 40)])
    n = hc.write_fasta(tmp_path / "nuc.fa", nuc + [("HLA:HLA16001", "DPB2*01:01:01:01", "ACGT" * 20), ("HLA:HLA20000", "DRB3*01:01:02:01", "ACGGT" * 10)])
    A = D.HlaAlleles.load(g, n)
    assert A.stats["n_dropped_gene"] == 1 and A.stats["n_alleles"] == 3 and "Removed 1 alleles" in A.stats["warnings"]
    assert [A.allele(i)["gene_name"] for i in range(3)] == ["HLA-A", "HLA-B", "HLA-DRB3"]           # a supported class II gene stays
    # HlaAlleleDefinition::new's own checks
    import __graft_entry__ as ge
    err = ge.load_package().StarphaseError
    for desc, seq, text in (("A01:01", "ACGT", "Star split length != 2 for allele description: A01:01"),
                            ("A*01:01:01:01:01", "ACGT", "Unexpected number of fields for allele description: A*01:01:01:01:01"),
                            ("A*01:02", "ACGNT", "cDNA sequence contains non-ACGT symbols.")):
        with pytest.raises(err, match=text.replace("*", r"\*")):
            D.HlaAlleles.load(hc.FAUX_GEN, hc.write_fasta(tmp_path / "bad.fa", nuc + [("HLA:HLA88888", desc, seq)]))
    with pytest.raises(err, match="cannot open"):
        D.HlaAlleles.load(hc.FAUX_GEN, tmp_path / "missing.fa")


def test_designed_set_maps_once_per_allele_in_the_oracle():
    """the GPU comparison (tests/test_gpu_hla_update.py) never rests on minimap2's multi-mapping order: every designed derivative that maps has exactly one
    mapping on its chosen strand in the restatement, the random sequences and the cDNA-only alleles have none, and the flanked alleles make the coordinates grow"""
    import test_oracle_mm2 as tm
    mm = tm.mm2_ffi.Mm2()
    S = hc.designed_set(mm)
    assert len(S) == 16
    ids = {a[2]: "HLA:HLA9%04d" % i for i, a in enumerate(S)}
    recs, genes = hc.oracle_extend(mm, S, ids, require_single=True)
    for gene, kind, desc, dna, _c in S:
        assert (recs[desc] is None) == (kind in ("random", "cdna_only")), (desc, kind)
    for gene, ((s, e), _want) in hc.REFSEQ.items():
        assert genes[gene][0] < s and genes[gene][2]
    assert (genes["HLA-A"][3], genes["HLA-B"][3]) == ("A*94:01:01:01", "B*94:01:01:01")


@pytest.mark.parametrize("gz", [False, True])
def test_save_hla_on_a_hand_made_result(D, tmp_path, gz):
    src = hc.refseq_database(variant_db="CACNA1S")
    src_path = tmp_path / "in.json"
    src_path.write_text(json.dumps(src))
    db = D.Database(src_path)
    A = D.HlaAlleles.load(hc.FAUX_GEN, hc.FAUX_NUC)
    coords = {"HLA-A": (29942253, 29945870), "HLA-B": (31353361, 31357442)}
    R = D.HlaConfigResult.make([(g, s, e) for g, (s, e) in coords.items()])
    out = tmp_path / ("out.json.gz" if gz else "out.json")
    db.save_hla(A, R, "3.58.0", out)
    raw = open(out, "rb").read()
    assert (raw[:2] == b"\x1f\x8b") == gz
    got = json.loads(gzip.decompress(raw) if gz else raw)
    assert list(got) == ["database_metadata", "gene_entries", "hla_config", "hla_sequences", "cyp2d6_gene_def"]              # PgxDatabase's member order
    assert got["hla_sequences"] == A.table() and list(got["hla_sequences"]) == ["HLA:HLA00001", "HLA:HLA00132"]
    assert list(got["hla_sequences"]["HLA:HLA00001"]) == ["hla_id", "gene_name", "star_allele", "dna_sequence", "cdna_sequence"]
    gd = got["hla_config"]["gene_collection"]["gene_dict"]
    assert got["hla_config"]["gene_collection"]["version"] == "NCBI RefSeq test"
    for g, (s, e) in coords.items():
        want = dict(src["hla_config"]["gene_collection"]["gene_dict"][g])
        want["coordinates"] = {"chrom": "chr6", "start": s, "end": e}
        assert gd[g] == want and list(gd[g]) == ["gene_name", "coordinates", "is_forward_strand", "transcript_id", "exons", "is_absent_capable"]
    assert got["database_metadata"] == dict(src["database_metadata"], hla_version="3.58.0")
    assert got["gene_entries"] == src["gene_entries"] and got["cyp2d6_gene_def"] == src["cyp2d6_gene_def"]
    again = D.Database(out)                                                                                                   # sp_database_load accepts it
    assert again.metadata["hla_version"] == "3.58.0" and again.stats.n_hla_sequences == 2 and again.stats.n_gene_entries == 1
    assert [(g["name"], g["start"], g["end"], len(g["exons"])) for g in again.hla_genes()] == [("HLA-A", 29942253, 29945870, 8), ("HLA-B", 31353361, 31357442, 8)]


def test_save_hla_from_a_database_without_hla_config_and_its_errors(D, pkg, tmp_path):
    db = D.Database(os.path.join(hc.GOLDEN, "hla_faux_database.json"))                 # no hla_config: the two-gene default, written in the v1.0 form
    A = D.HlaAlleles.load(hc.FAUX_GEN, hc.FAUX_NUC)
    db.save_hla(A, D.HlaConfigResult.make([("HLA-A", 29942200, 29945900), ("HLA-B", 31353361, 31357442)]), "x", tmp_path / "o.json")
    got = json.load(open(tmp_path / "o.json"))
    a = got["hla_config"]["gene_collection"]["gene_dict"]["HLA-A"]
    assert a["coordinates"] == {"chrom": "chr6", "start": 29942200, "end": 29945900} and a["transcript_id"] == "NM_002116.8" and len(a["exons"]) == 8
    assert D.Database(tmp_path / "o.json").hla_genes()[0]["start"] == 29942200
    with pytest.raises(pkg.StarphaseError, match="no definition for HLA-C"):
        db.save_hla(A, D.HlaConfigResult.make([("HLA-C", 1, 2)]), "x", tmp_path / "p.json")
    with pytest.raises(pkg.StarphaseError, match="cannot open"):
        db.save_hla(A, D.HlaConfigResult.make([("HLA-A", 1, 2)]), "x", tmp_path / "no_such_dir" / "p.json")

"""Files to files on the GPU: sp_starphase_create / sp_starphase_call (call_diplotypes, src/diplotyper.rs:40-330) and the `starphase_hip diplotype`
command against the step-by-step ABI path, the reference's scenario tables and the simulated truth."""
import gzip
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import cyp_cases_real as cr
import test_io
from test_oracle_variant import CASES, SV_CASES

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VCF_DIR = os.path.join(GOLDEN, "vcf")


def genome_fasta(path, extra=None):
    """test_reference.json (the reference's test genome) as an indexed FASTA, plus any extra contigs"""
    seqs = json.load(open(os.path.join(GOLDEN, "test_reference.json")))
    seqs.update(extra or {})
    test_io.write_fasta(path, seqs, 60, index=True)
    return str(path)


def same_dips(got, want):
    """Diplotype equality ignores the haplotype order (src/data_types/pgx_diplotype.rs:67-73); the list order matters"""
    key = lambda d: frozenset(d) if d[0] != d[1] else d
    return [key(d) for d in got] == [key(d) for d in want]


def inexact_sets(entry):
    out = []
    for x in entry["inexact_diplotypes"] or []:
        sides = []
        for h in (x["haplotype_1"], x["haplotype_2"]):
            sides.append((h["base_haplotype"], {(v["label"], v["is_vi"], v["variant_state"]) for v in h["variant_relationships"]}))
        out.append(tuple(sides))
    return out


# ------------------------------------------------------------------ 1. variant genes from files
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[1])
def test_variant_gene_scenarios_from_files(pkg, oracle, tmp_path, case):
    import variant_glue as vg
    db_name, vcf, with_ref, dips, inexact = case
    db_path = os.path.join(GOLDEN, "variant_dbs", db_name + ".json")
    fasta = genome_fasta(tmp_path / "ref.fa") if with_ref else None
    sp = pkg.database.Starphase(db_path, fasta)
    got = json.loads(sp.call(vcf=os.path.join(VCF_DIR, vcf)).json())
    gene, prob = vg.load_case(oracle, db_name, vcf, with_ref)
    e = got["gene_details"][gene]
    assert same_dips([(d["hap1"], d["hap2"]) for d in e["diplotypes"]], dips)
    want = vg.call_gene(oracle, prob)                           # the test glue's packaging of the same solve
    if inexact is None:
        assert e["inexact_diplotypes"] is None
    else:
        assert inexact_sets(e) == [((a, set(ra)), (b, set(rb))) for (a, ra), (b, rb) in inexact]
    assert [(d["hap1"], d["hap2"]) for d in e["diplotypes"]] == [tuple(d) for d in want["diplotypes"]]
    if want["simple"] is not None and e["simple_diplotypes"] is not None:
        assert [(d["hap1"], d["hap2"]) for d in e["simple_diplotypes"]] == [tuple(d) for d in want["simple"]]
    # variant_details: the observed variants in NormalizedVariant order, with their genotypes
    nv = [v["normalized_variant"] for v in e["variant_details"]]
    assert [(v["chrom"], v["position"], v["reference"], v["alternate"]) for v in nv] == [tuple(o) for o in prob.obs]
    gt = {1: "0/1", 2: "0|1", 3: "1|0", 4: "1/1"}
    assert [v["normalized_genotype"]["genotype"] for v in e["variant_details"]] == [gt[int(g)] for g in prob.obs_gt[:len(prob.obs)]]
    sp.close()


@pytest.mark.parametrize("case", SV_CASES, ids=lambda c: c[0])
def test_variant_gene_sv_vcf_from_files(pkg, tmp_path, case):
    sv_vcf, dips, _inexact = case
    sp = pkg.database.Starphase(os.path.join(GOLDEN, "variant_dbs", "DPYD-sv-test.json"), genome_fasta(tmp_path / "ref.fa"),
                                sv_vcf=os.path.join(VCF_DIR, sv_vcf))
    e = json.loads(sp.call(vcf=os.path.join(VCF_DIR, "DPYD-sv-test/empty_small.vcf.gz")).json())["gene_details"]["DPYD"]
    assert [(d["hap1"], d["hap2"]) for d in e["diplotypes"]] == dips
    svs = [v for v in e["variant_details"] if v["variant_name"] == "structural_variant"]
    assert len(svs) == 2 and all(v["variant_id"] == 2 ** 64 - 1 for v in svs)
    sp.close()


# ------------------------------------------------------------------ 2. a whole sample from files
class Sample:
    """database (HLA-A/-B, CYP2D6, two variant genes), reference FASTA, two BAMs, a VCF -- and the truth they were drawn from"""

    def __init__(self, root, pkg, seed=41):
        from pb_starphase_amd import synth
        rng = np.random.default_rng(seed)
        self.root = root
        db = {}
        for f in ("hla_db_v0.14.1.json.gz", "cyp2d6_db_v0.14.1.json.gz"):
            db.update(json.load(gzip.open(os.path.join(GOLDEN, f))))
        ge = {}
        for name in ("UGT1A1-faux", "CYP2C8-faux"):
            ge.update(json.load(open(os.path.join(GOLDEN, "variant_dbs", name + ".json")))["gene_entries"])
        db["gene_entries"] = ge
        self.db = str(root / "db.json")
        json.dump(db, open(self.db, "w"))
        # reference: chr2 / chr3 of the test genome, chr6 with the HLA islands, chr22 with the CYP2D6 window
        fx = self.fx = synth.HlaFixture()
        cfg, gene_def = cr.load_db()
        self.locus = locus = synth.Chr22Locus(cfg, gene_def, seed=3)
        chr6 = bytearray(b"N" * (max(e for _s, e in fx.coords) + fx.buffer + 20000))
        for (s0, _e0), ref in zip(fx.coords, fx.gene_ref):
            chr6[s0 - fx.buffer:s0 - fx.buffer + len(ref)] = ref.encode()
        chr22 = bytearray(b"N" * (locus.start + len(locus.sequence) + 1000))
        chr22[locus.start:locus.start + len(locus.sequence)] = locus.sequence.encode()
        self.fasta = genome_fasta(root / "ref.fa", {"chr6": chr6.decode(), "chr22": chr22.decode()})
        self.refs = [("chr6", len(chr6)), ("chr22", len(chr22))]
        # HLA reads of two alleles per gene; CYP2D6 reads of *4/*4
        self.hla_truth, hla_reads = {}, []
        for g in range(len(fx.genes)):
            pick = rng.choice(fx.full_length_alleles(g), 2, replace=False).tolist()
            self.hla_truth[fx.genes[g]] = pick
            for a in pick:
                hap, s = fx.haplotype(g, a)
                hla_reads += [(g, r) for r in synth.simulate_reads(rng, hap, s, len(fx.dna[a]), 23, mean_len=6000, sd_len=1500, min_overlap=2500)]
        _n, haps, self.cyp_truth = cr.scenarios(locus)[1]
        cyp_reads = locus.sample(rng, haps, 120, lo=8000, hi=16000)
        self.hla_reads, self.cyp_reads = hla_reads, cyp_reads
        recs = []
        for i in rng.permutation(len(hla_reads)).tolist():
            g, seq = hla_reads[i]
            recs.append((0, fx.coords[g][0] + int(rng.integers(-3000, 2000)), f"m84/{i}/ccs", 0, 60, [("M", len(seq))], seq))
        d6 = cfg["cyp_coordinates"]["CYP2D6"]
        for i, seq in enumerate(cyp_reads):
            recs.append((1, d6["start"] + int(rng.integers(-8000, 2000)), f"m84/cyp{i:03d}/ccs", 0, 60, [("M", len(seq))], seq))
        # a read far from every region (never fetched) and a secondary record of a read that also has its primary (first record wins)
        recs.append((0, 1000, "m84/outside/ccs", 0, 60, [("M", 5000)], "ACGT" * 1250))
        recs.append((0, fx.coords[0][0] + 2500, recs[0][2], 256, 0, [("M", len(recs[0][6]))], recs[0][6]))
        # reads of HLA-A on the reverse strand: K1 accepts them reverse and the reference ignores them, naming the allele (realigner.rs:178-193)
        for i in range(3):
            seq = synth.revcomp(hla_reads[i][1])
            recs.append((0, fx.coords[0][0] + 100 * i, f"m84/rev{i}/ccs", 0, 60, [("M", len(seq))], seq))
        # two BAMs: every third record is in the second file, and a few QNAMEs are in both
        first = [r for k, r in enumerate(recs) if k % 3 != 0]
        # a secondary record without SEQ ('*') that comes before its primary: the first record of the QNAME wins, an empty read
        # (realigner.rs:111-114: no mappings, ignored as REFERENCE with MappingStats(0, 0, 0))
        only_second = [r for k, r in enumerate(recs) if k % 3 == 0]
        prim = next(r for r in only_second if r[0] == 0 and r[3] == 0 and "/rev" not in r[2] and r[2] != "m84/outside/ccs")
        self.seqless = prim[2]
        first.append((0, fx.coords[0][0] + 10, prim[2], 256, 0, [("M", 1000)], ""))      # in the first BAM, inside HLA-A: met before the primary
        second = [r for k, r in enumerate(recs) if k % 3 == 0] + first[:10]
        self.bams = []
        for name, part in (("a.bam", first), ("b.bam", second)):
            path = str(root / name)
            test_io.write_bam(path, self.refs, sorted(part, key=lambda r: (r[0], r[1], r[2])), 65280)
            self.bams.append(path)
        self.recs_by_file = [sorted(first, key=lambda r: (r[0], r[1], r[2])), sorted(second, key=lambda r: (r[0], r[1], r[2]))]
        # a hla-only BAM (no CYP2D6 reads)
        self.hla_bam = str(root / "hla_only.bam")
        test_io.write_bam(self.hla_bam, self.refs, sorted([r for r in recs if r[0] == 0 and r[3] == 0], key=lambda r: (r[0], r[1], r[2])), 65280)
        # the VCF: UGT1A1 opposite_phase_001 with a second sample column in front
        self.vcf = os.path.join(VCF_DIR, "UGT1A1-faux", "opposite_phase_001.vcf.gz")
        self.vcf2 = str(root / "two_samples.vcf")
        lines = gzip.open(self.vcf, "rt").read().splitlines()
        out = []
        for ln in lines:
            if ln.startswith("##"):
                out.append(ln)
            elif ln.startswith("#"):
                c = ln.split("\t")
                out.append("\t".join(c[:9] + ["OTHER"] + c[9:]))
            else:
                c = ln.split("\t")
                out.append("\t".join(c[:9] + ["0/0" + c[9][3:]] + c[9:]))
        open(self.vcf2, "w").write("\n".join(out) + "\n")
        self.sample_name = [ln for ln in lines if ln.startswith("#CHROM")][0].split("\t")[9]


@pytest.fixture(scope="module")
def sample(pkg, tmp_path_factory):
    return Sample(tmp_path_factory.mktemp("sample"), pkg)


@pytest.fixture(scope="module")
def handle(pkg, sample):
    h = pkg.database.Starphase(sample.db, sample.fasta)
    yield h
    h.close()


def fetch_order(sample, regions, D):
    """the read loop of the reference: regions in order, every BAM in the given order, a QNAME once; no FLAG filter"""
    seen, out = set(), []
    for g, (chrom, s, e) in enumerate(regions):
        for path in sample.bams:
            for r in D.Bam(path).fetch(chrom, s, e, exclude_flags=0, dedupe=False):
                if r["qname"] not in seen:
                    seen.add(r["qname"])
                    out.append((g, r["qname"], r["seq"]))
    return out


def test_whole_sample_from_files(pkg, gpu_ctx, sample, handle):
    D = pkg.database
    res = handle.call(bams=sample.bams, vcf=sample.vcf)
    got = json.loads(res.json())["gene_details"]
    assert sorted(got) == ["CYP2C8", "CYP2D6", "HLA-A", "HLA-B", "UGT1A1"]
    # variant genes: the reference's scenario table
    assert same_dips([(d["hap1"], d["hap2"]) for d in got["UGT1A1"]["diplotypes"]], [("*28", "*80")])
    # CYP2D6: the simulated truth and the step-by-step path on the same reads in QNAME order
    d6 = got["CYP2D6"]
    assert sorted([d6["diplotypes"][0]["hap1"], d6["diplotypes"][0]["hap2"]]) == sorted(sample.cyp_truth)
    dbf = D.Database(sample.db)
    w_chrom, _ws, _we = dbf.cyp_window()
    fasta = D.Fasta(sample.fasta)
    cdb = dbf.cyp_db(gpu_ctx, fasta.fetch(w_chrom, sample.locus.start, sample.locus.start + len(sample.locus.sequence)), sample.locus.start)
    cfg, _gd = cr.load_db()
    ext = (min(cfg["cyp_coordinates"][k]["start"] for k in ("CYP2D6", "CYP2D7", "REP6", "REP7")),)
    s5 = cfg["cyp2d6_star5_del"]
    lo = min(ext[0], s5["start"] - 500)
    hi = max(max(cfg["cyp_coordinates"][k]["end"] for k in ("CYP2D6", "CYP2D7", "REP6", "REP7")), s5["end"] + 3000)
    cyp_reads = sorted(fetch_order(sample, [("chr22", lo, hi)], D), key=lambda x: x[1])
    assert len(cyp_reads) == len(sample.cyp_reads)
    call, _c, _l = cdb.diplotype(gpu_ctx.upload([r[2] for r in cyp_reads]))
    assert (d6["diplotypes"][0]["hap1"], d6["diplotypes"][0]["hap2"]) == (call.hap1.decode(), call.hap2.decode())
    assert (d6["simple_diplotypes"][0]["hap1"], d6["simple_diplotypes"][0]["hap2"]) == (call.core1.decode(), call.core2.decode())
    # HLA: the simulated truth, the step-by-step path, and every mapping_details entry re-derived from the sp_hla_realign records
    regions = dbf.hla_genes()
    gene_ref = [fasta.fetch(r["chrom"], r["start"] - 100, r["end"] + 100) for r in regions]
    hdb, alleles = dbf.hla_db(gpu_ctx, gene_ref)
    met = fetch_order(sample, [(r["chrom"], r["start"], r["end"]) for r in regions], D)
    by_q = sorted(met, key=lambda x: x[1])
    R = gpu_ctx.upload([x[2] for x in by_q])
    rec = hdb.realign_reads(R)
    calls, _ = hdb.diplotype_genes(list(range(len(regions))), R, rec)
    star = lambda a: "." if a == -2 else ("" if a < 0 else "*" + alleles[a][2])
    pos = {q: k for k, (_g, q, _s) in enumerate(by_q)}
    for g, (c, _c1, _c2) in enumerate(calls):
        name = regions[g]["name"]
        e = got[name]
        assert c.status == 0 and [(d["hap1"], d["hap2"]) for d in e["diplotypes"]] == [(star(c.allele1), star(c.allele2))]
        truth = sorted(sample.hla_truth[name])
        fx = sample.fx
        same = lambda a, b: a == b or (fx.cdna[a] == fx.cdna[b] and fx.dna[a] == fx.dna[b])
        gi = sorted([fx.ids.index(alleles[c.allele1][0]), fx.ids.index(alleles[c.allele2][0])])
        assert all(same(a, b) for a, b in zip(gi, truth)) or all(same(a, b) for a, b in zip(gi, truth[::-1])), (name, gi, truth)
        want = []
        for sg, q, seq in met:
            r = rec[pos[q]]
            realigned = r["status"] == 0
            if (int(r["gene"]) if realigned else sg) != g:
                continue
            if r["status"] == 2 and r["best_allele"] < 0:
                # accepted on the reverse strand: the audit's mapping in minimap2's output order that the acceptance loop keeps (realigner.rs:124-146)
                au = hdb.realign_seeded_audit(R, pos[q])
                best, pick = 1.0, None
                for hit in au["hits"]:
                    tl, um, nm = int(hit["t_len"]), int(hit["t_len"]) - (int(hit["t_end"]) - int(hit["t_start"])), int(hit["nm"])
                    if tl > 0 and tl - um > 0 and max(0.1, nm + um) / tl <= 0.5 and max(0.1, nm) / (tl - um) <= 0.03 and max(0.1, nm) / (tl - um) < best:
                        best, pick = max(0.1, nm) / (tl - um), hit
                assert pick is not None and int(pick["rev"]) == 1
                a = int(pick["allele"])
                stats = {"seq_len": int(pick["t_len"]), "nm": int(pick["nm"]), "unmapped": int(pick["t_len"]) - (int(pick["t_end"]) - int(pick["t_start"]))}
                ident = (alleles[a][0], f"{alleles[a][1]}*{alleles[a][2]}")
            elif r["best_allele"] >= 0 and r["status"] != 1:
                a = int(r["best_allele"])
                stats = {"seq_len": int(r["target_len"]), "nm": int(r["mm2_nm"]),
                         "unmapped": max(0, int(r["target_len"]) - (int(r["mm2_t_end"]) - int(r["mm2_t_start"]))), "clipped": None}
                ident = (alleles[a][0], f"{alleles[a][1]}*{alleles[a][2]}")
            else:
                stats, ident = {"seq_len": len(seq), "nm": len(seq), "unmapped": 0, "clipped": None}, ("REFERENCE", "REFERENCE")
            want.append((q, ident[0], ident[1], stats, not realigned))
        md = e["mapping_details"]
        assert len(md) == len(want) > 0
        for m, (q, hid, st, stats, ign) in zip(md, want):
            assert (m["read_qname"], m["best_hla_id"], m["best_star_allele"], m["is_ignored"]) == (q, hid, st, ign)
            dna = m["best_mapping_stats"]["dna_stats"]
            assert (dna["seq_len"], dna["nm"], dna["unmapped"]) == (stats["seq_len"], stats["nm"], stats["unmapped"]), q
    # the fixture's edge cases reached the entry: reverse-strand reads named after their allele, the SEQ-less record as an empty ignored read
    by_name = {m["read_qname"]: m for n in ("HLA-A", "HLA-B") for m in got[n]["mapping_details"]}
    revs = [by_name[f"m84/rev{i}/ccs"] for i in range(3)]
    assert all(m["is_ignored"] and m["best_hla_id"] != "REFERENCE" and m["best_star_allele"].startswith("HLA-A*") for m in revs), revs
    assert all(m["best_mapping_stats"]["dna_stats"]["seq_len"] > 0 and
               m["best_mapping_stats"]["dna_stats"]["nm"] <= 0.03 * m["best_mapping_stats"]["dna_stats"]["seq_len"] for m in revs), revs
    empty = by_name[sample.seqless]
    assert empty["is_ignored"] and empty["best_hla_id"] == "REFERENCE" and \
        (empty["best_mapping_stats"]["dna_stats"]["seq_len"], empty["best_mapping_stats"]["dna_stats"]["nm"]) == (0, 0)
    # CYP2D6 multi_mapping_details: the reads with exactly one chain, each region inside its read; equal to sp_cyp_diplotype_mappings on the same reads
    mm = d6["multi_mapping_details"]
    assert len(mm) > 0
    call2, maps = D.cyp_diplotype_mappings(cdb, gpu_ctx.upload([r[2] for r in cyp_reads]))
    assert (call2.hap1, call2.hap2) == (call.hap1, call.hap2)
    assert [(m["read_qname"], m["read_position"]["start"], m["read_position"]["end"], m["consensus_id"], m["consensus_star_allele"]) for m in mm] == \
        [(cyp_reads[r][1], s, e, c, lab) for r, s, e, c, lab in maps]
    seq_of = {q: s for _g, q, s in cyp_reads}
    per_read = {}
    for m in mm:
        per_read.setdefault(m["read_qname"], []).append(m)
        assert 0 <= m["read_position"]["start"] < m["read_position"]["end"] <= len(seq_of[m["read_qname"]]), m
        assert m["consensus_star_allele"].startswith(f"{m['consensus_id']}_"), m
    for q, ms in per_read.items():          # one chain per read: its regions in read order, each consensus once per region
        starts = [m["read_position"]["start"] for m in ms]
        assert starts == sorted(starts) and len(ms) <= len(seq_of[q]) // 1000 + 2, (q, ms)
    assert list(per_read) == sorted(per_read)                           # QNAME (BTreeMap) order
    t = handle.timing()
    assert t["n_hla_reads"] == len(met) and t["n_cyp_reads"] == len(sample.cyp_reads) and t["bam_decode_ms"] > 0
    print("\nwhole-sample timing:", json.dumps(t))


# ------------------------------------------------------------------ 3. options and edge cases
def test_options_and_edge_cases(pkg, sample, handle, tmp_path):
    D = pkg.database
    # include / exclude sets (made once per handle)
    inc = tmp_path / "include.txt"; inc.write_text("UGT1A1\nHLA-B\n")
    exc = tmp_path / "exclude.txt"; exc.write_text("CYP2D6\nHLA-A\nCYP2C8\n")
    h = D.Starphase(sample.db, sample.fasta, include_set=str(inc))
    assert sorted(json.loads(h.call(bams=sample.bams, vcf=sample.vcf).json())["gene_details"]) == ["HLA-B", "UGT1A1"]
    h.close()
    h = D.Starphase(sample.db, sample.fasta, exclude_set=str(exc))
    assert sorted(json.loads(h.call(bams=sample.bams, vcf=sample.vcf).json())["gene_details"]) == ["HLA-B", "UGT1A1"]
    h.close()
    # the sample of a two-sample VCF: by name, and the first one by default
    named = json.loads(handle.call(vcf=sample.vcf2, sample_name=sample.sample_name).json())["gene_details"]
    assert same_dips([(d["hap1"], d["hap2"]) for d in named["UGT1A1"]["diplotypes"]], [("*28", "*80")])
    first = json.loads(handle.call(vcf=sample.vcf2).json())["gene_details"]
    assert [(d["hap1"], d["hap2"]) for d in first["UGT1A1"]["diplotypes"]] == [("*1", "*1")]
    # no BAM: variant genes only; no VCF: BAM genes only
    assert sorted(json.loads(handle.call(vcf=sample.vcf).json())["gene_details"]) == ["CYP2C8", "UGT1A1"]
    assert sorted(json.loads(handle.call(bams=sample.bams).json())["gene_details"]) == ["CYP2D6", "HLA-A", "HLA-B"]
    # no CYP2D6 reads: the reference's NO_READS entry (src/cyp2d6/caller.rs:254-266)
    d6 = json.loads(handle.call(bams=[sample.hla_bam]).json())["gene_details"]["CYP2D6"]
    assert d6["diplotypes"] == [{"hap1": "NO_READS", "hap2": "NO_READS", "diplotype": "NO_READS/NO_READS"}]
    assert d6["simple_diplotypes"] is None and d6["inexact_diplotypes"] is None and d6["multi_mapping_details"] == []


# ------------------------------------------------------------------ 4. determinism
def test_sequential_and_overlapped_runs_agree(pkg, sample, handle):
    D = pkg.database
    over = handle.call(bams=sample.bams, vcf=sample.vcf).json()
    seq_h = D.Starphase(sample.db, sample.fasta, sequential=1)
    assert seq_h.call(bams=sample.bams, vcf=sample.vcf).json() == over
    t_seq = seq_h.timing()
    seq_h.close()
    # three samples through one handle == three fresh handles
    inputs = [dict(bams=sample.bams, vcf=sample.vcf), dict(bams=[sample.hla_bam], vcf=sample.vcf2), dict(vcf=sample.vcf2, sample_name=sample.sample_name)]
    through = [handle.call(**kw).json() for kw in inputs]
    for kw, want in zip(inputs, through):
        h = D.Starphase(sample.db, sample.fasta)
        assert h.call(**kw).json() == want
        h.close()
    print("\nsequential timing:", json.dumps(t_seq))


# ------------------------------------------------------------------ 5. the command line on the GPU
def test_cli_files_equal_the_api(pkg, sample, handle, tmp_path):
    import time
    D = pkg.database
    out, tsv, dbg = tmp_path / "calls.json", tmp_path / "calls.tsv", tmp_path / "debug"
    api_dbg = tmp_path / "api_debug"
    t0 = time.time()
    h = D.Starphase(sample.db, sample.fasta, debug_folder=str(api_dbg))
    t_create = time.time() - t0
    res = h.call(bams=sample.bams, vcf=sample.vcf)
    res.save(str(tmp_path / "api.json")); res.save_pharmcat_tsv(str(tmp_path / "api.tsv"))
    h.close()
    cmd = [D.cli_path(), "diplotype", "-d", sample.db, "-r", sample.fasta, "-c", sample.vcf, "-b", sample.bams[0], "--bam", sample.bams[1],
           "-o", str(out), "--pharmcat-tsv", str(tsv), "--output-debug", str(dbg), "-v"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert out.read_bytes() == (tmp_path / "api.json").read_bytes()
    assert tsv.read_bytes() == (tmp_path / "api.tsv").read_bytes()
    assert sorted(os.listdir(dbg)) == sorted(os.listdir(api_dbg)) == ["cyp2d6_alleles.json", "hla_debug.json"]
    for f in os.listdir(dbg):
        assert (dbg / f).read_bytes() == (api_dbg / f).read_bytes(), f
    print(f"\nsp_starphase_create: {t_create * 1000:.0f} ms; CLI: {p.stderr.strip().splitlines()[-1]}")
    shutil.rmtree(dbg)

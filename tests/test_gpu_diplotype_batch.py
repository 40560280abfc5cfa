"""Many samples from files on the GPU: sp_starphase_call_batch / Starphase.call_batch and `starphase_hip diplotype-batch` against single
sp_starphase_call runs on the same handle (byte for byte, for every group size and decode thread count), and the library pieces the batch is made
of: sp_hla_realign_reads_rev against sp_hla_realign_reads plus the seeded audit, sp_hla_diplotype_cohort_samples against sp_hla_diplotype_gene,
sp_cyp_diplotype_cohort_mappings against sp_cyp_diplotype_mappings."""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

import cyp_cases_real as cr
from test_gpu_diplotype_files import Sample, fetch_order

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cohort(pkg, tmp_path_factory):
    """eight simulated samples (distinct seeds: other HLA truths, other reads) sharing one database and reference"""
    return [Sample(tmp_path_factory.mktemp(f"s{k}"), pkg, seed=41 + 17 * k) for k in range(8)]


@pytest.fixture(scope="module")
def handle(pkg, cohort):
    h = pkg.database.Starphase(cohort[0].db, cohort[0].fasta)
    yield h
    h.close()


def batch_inputs(cohort, tmp_path):
    s = cohort
    return [dict(bams=s[0].bams, vcf=s[0].vcf),                                            # reverse-strand reads and a SEQ-less record
            dict(bams=s[1].bams, vcf=s[1].vcf2, sample_name=s[1].sample_name),
            dict(vcf=s[2].vcf2),                                                          # VCF only (the first sample of the file)
            dict(bams=s[3].bams),                                                         # BAMs only
            dict(bams=[s[4].hla_bam], vcf=s[4].vcf),                                      # no reads in the CYP2D6 region
            dict(bams=[s[5].bams[0], str(tmp_path / "missing.bam")], vcf=s[5].vcf),       # fails alone
            dict(bams=[s[6].bams[1], s[6].bams[0]], vcf=s[6].vcf),
            dict(bams=s[7].bams, vcf=s[7].vcf),
            dict(vcf=s[0].vcf, sample_name="NOT_IN_THE_VCF")]                             # fails alone


def single(handle, inputs):
    out = []
    for kw in inputs:
        try:
            r = handle.call(**kw)
            out.append((r.json(), r.pharmcat_tsv()))
        except Exception as e:              # noqa: BLE001 -- the failure is what is compared
            out.append(e)
    return out


def test_batch_equals_single_calls(pkg, cohort, handle, tmp_path):
    D = pkg.database
    inputs = batch_inputs(cohort, tmp_path)
    want = single(handle, inputs)
    assert [i for i, w in enumerate(want) if isinstance(w, Exception)] == [5, 8]
    runs = {}
    for max_group, threads in ((None, None), (1, 1), (3, 8), (len(inputs), 1), (len(inputs), 8), (2, 3)):
        t0 = time.time()
        got = handle.call_batch(inputs, max_group=max_group, threads=threads)
        runs[(max_group, threads)] = time.time() - t0
        assert len(got) == len(inputs)
        for i, (g, w) in enumerate(zip(got, want)):
            if isinstance(w, Exception):
                assert isinstance(g, D.StarphaseError), (i, g)
                assert (g.code, str(g)) == (w.code, str(w)), (i, str(g), str(w))
            else:
                assert not isinstance(g, Exception), (i, g)
                assert (g.json(), g.pharmcat_tsv()) == w, (i, max_group, threads)
        t = handle.batch_timing()
        assert t["n_samples"] == len(inputs) and t["n_failed"] == 2
        assert t["n_groups"] == (1 if max_group is None else -(-len(inputs) // max_group))
    assert "missing.bam" in str(got[5])
    print("\nbatch wall times (s):", runs)


def test_batch_debug_files_equal_single_calls(pkg, cohort, tmp_path):
    D = pkg.database
    s0 = cohort[0]
    inputs = [dict(bams=c.bams, vcf=c.vcf) for c in cohort[:3]] + [dict(bams=[cohort[3].hla_bam])]
    h = D.Starphase(s0.db, s0.fasta, debug_folder=str(tmp_path / "single"))
    want = []
    for i, kw in enumerate(inputs):
        r = h.call(**kw)
        want.append(r.json())
        shutil.copytree(tmp_path / "single", tmp_path / f"want{i}")
        shutil.rmtree(tmp_path / "single")
    # a handle with a debug folder: the batch needs a folder per sample
    with pytest.raises(D.StarphaseError) as e:
        h.call_batch(inputs)
    assert e.value.code == 1 and "debug" in str(e.value)                        # SP_ERR_INVALID_ARG
    folders = [str(tmp_path / f"got{i}") for i in range(len(inputs))]
    got = h.call_batch(inputs, max_group=3, debug_folders=folders)
    for i in range(len(inputs)):
        assert got[i].json() == want[i]
        assert sorted(os.listdir(folders[i])) == sorted(os.listdir(tmp_path / f"want{i}")), i
        for f in os.listdir(folders[i]):
            assert open(os.path.join(folders[i], f), "rb").read() == open(tmp_path / f"want{i}" / f, "rb").read(), (i, f)
    assert sorted(os.listdir(folders[0])) == ["cyp2d6_alleles.json", "hla_debug.json"]
    h.close()


def test_hla_failure_stays_with_its_sample(pkg, cohort, handle, tmp_path):
    """a sample whose HLA lane fails (its debug folder is a file: hla_debug.json cannot be written) fails as its single call does, with the same
    text and no warnings, and the samples it shares the group with are still typed, byte for byte"""
    D = pkg.database
    bad = tmp_path / "not_a_folder"
    bad.write_text("")
    inputs = [dict(bams=cohort[0].bams, vcf=cohort[0].vcf), dict(bams=cohort[2].bams, vcf=cohort[2].vcf), dict(bams=cohort[3].bams)]
    want = single(handle, inputs)
    h_bad = D.Starphase(cohort[0].db, cohort[0].fasta, debug_folder=str(bad))
    with pytest.raises(D.StarphaseError) as e:
        h_bad.call(**inputs[1])
    h_bad.close()
    assert "hla_debug.json" in str(e.value)
    for max_group in (None, 2):
        got = handle.call_batch(inputs, max_group=max_group, debug_folders=[None, str(bad), None])
        assert isinstance(got[1], D.StarphaseError) and (got[1].code, str(got[1])) == (e.value.code, str(e.value)), str(got[1])
        assert handle.sample_warnings(1) == ""
        for i in (0, 2):
            assert (got[i].json(), got[i].pharmcat_tsv()) == want[i], (i, max_group)


def test_exhaustive_k1_context_single_and_batch_agree(pkg, cohort, k1_exhaustive):
    """a handle on a caller's context in exhaustive K1 mode (k1_best_n = 0): both entry points run, give the same bytes, and the reverse-strand
    reads are ignored (no seeded stage names a mapping for them)"""
    import json
    h = pkg.database.Starphase(cohort[0].db, cohort[0].fasta, ctx=k1_exhaustive)
    try:
        inputs = [dict(bams=c.bams, vcf=c.vcf) for c in cohort[:2]]
        want = [h.call(**kw) for kw in inputs]
        got = h.call_batch(inputs)
        for i, (g, w) in enumerate(zip(got, want)):
            assert not isinstance(g, Exception), (i, g)
            assert (g.json(), g.pharmcat_tsv()) == (w.json(), w.pharmcat_tsv()), i
            details = json.loads(w.json())["gene_details"]
            by_name = {m["read_qname"]: m for n in ("HLA-A", "HLA-B") for m in details[n]["mapping_details"]}
            assert all(by_name[f"m84/rev{k}/ccs"]["is_ignored"] for k in range(3)), i
    finally:
        h.close()


def test_batch_variant_problems_stay_with_their_sample(pkg, tmp_path):
    """samples of one group with different records for the same gene, two of them structural variants given per sample: each entry is packaged from
    its own sample's problem (ids, deletion labels), so it equals that sample's single call, whatever the order in the group"""
    import json
    from test_gpu_diplotype_files import GOLDEN, VCF_DIR, genome_fasta
    from test_oracle_variant import SV_CASES
    small = os.path.join(VCF_DIR, "DPYD-sv-test/empty_small.vcf.gz")
    h = pkg.database.Starphase(os.path.join(GOLDEN, "variant_dbs", "DPYD-sv-test.json"), genome_fasta(tmp_path / "ref.fa"))
    try:
        inputs = [dict(vcf=small, sv_vcf=os.path.join(VCF_DIR, sv)) for sv, _d, _i in SV_CASES] + [dict(vcf=small)]
        want = [h.call(**kw) for kw in inputs]
        dips = [[(d["hap1"], d["hap2"]) for d in json.loads(w.json())["gene_details"]["DPYD"]["diplotypes"]] for w in want]
        assert dips[:2] == [d for _s, d, _i in SV_CASES] and dips[0] != dips[1] != dips[2]
        n_sv = [sum(v["variant_name"] == "structural_variant" for v in json.loads(w.json())["gene_details"]["DPYD"]["variant_details"]) for w in want]
        assert n_sv == [2, 2, 0]
        for order in ([0, 1, 2], [2, 1, 0], [1, 0, 2, 0, 1]):
            got = h.call_batch([inputs[k] for k in order])
            for g, k in zip(got, order):
                assert not isinstance(g, Exception), (order, k, g)
                assert (g.json(), g.pharmcat_tsv()) == (want[k].json(), want[k].pharmcat_tsv()), (order, k)
    finally:
        h.close()


# ------------------------------------------------------------------ the pieces
def hla_reads(sample):
    """the fixture's HLA reads plus reverse complements of some of them (K1 drops those on the reverse strand)"""
    from pb_starphase_amd import synth
    seqs = [r for _g, r in sample.hla_reads]
    return seqs + [synth.revcomp(seqs[i]) for i in range(0, len(seqs), 5)]


def audit_rev(db, gpu_ctx, seqs, rec):
    """the per-read statement of the reverse mappings: the status-2 reads alone, one seeded audit each, realign_record's acceptance rule over the mappings"""
    want = {}
    pos = [k for k in range(len(rec)) if rec["status"][k] == 2 and rec["best_allele"][k] < 0]
    if not pos:
        return want, pos
    sub = gpu_ctx.upload([seqs[k] for k in pos])
    for i, k in enumerate(pos):
        a = db.realign_seeded_audit(sub, i, chain_cap=256)
        best, b = 1.0, -1
        for x, h in enumerate(a["hits"]):
            tl, um, nm = int(h["t_len"]), int(h["t_len"] - (h["t_end"] - h["t_start"])), int(h["nm"])
            if tl <= 0 or tl - um <= 0:
                continue
            pen, ed = max(0.1, nm + um) / tl, max(0.1, nm) / (tl - um)
            if pen <= 0.5 and ed <= 0.03 and ed < best:
                best, b = ed, x
        if b >= 0 and a["hits"][b]["rev"] and a["hits"][b]["allele"] >= 0:
            h = a["hits"][b]
            want[k] = (int(h["allele"]), int(h["t_len"]), int(h["nm"]), int(h["t_start"]), int(h["t_end"]))
    return want, pos


def test_realign_reads_rev_equals_realign_and_audit(pkg, gpu_ctx, cohort, monkeypatch):
    from pb_starphase_amd import synth
    fx = synth.HlaFixture()
    db = fx.make_db(pkg, gpu_ctx)
    seqs = hla_reads(cohort[0]) + hla_reads(cohort[1])
    R = gpu_ctx.upload(seqs)
    plain = db.realign_reads(R)
    rec, rev = db.realign_reads_rev(R)
    assert rec.tobytes() == plain.tobytes()
    want, pos = audit_rev(db, gpu_ctx, seqs, rec)
    assert len(pos) >= 5 and len(want) >= 5, (len(pos), len(want))
    for k in range(len(seqs)):
        if k in want:
            assert (rev["allele"][k], rev["t_len"][k], rev["nm"][k], rev["t_start"][k], rev["t_end"][k]) == want[k], k
        else:
            assert rev["allele"][k] == -1, k
    # a set larger than the K1 slice: the same records and reverse mappings
    monkeypatch.setenv("SP_K1_SLICE", "7")
    rec2, rev2 = db.realign_reads_rev(R)
    monkeypatch.delenv("SP_K1_SLICE")
    assert rec2.tobytes() == rec.tobytes() and rev2.tobytes() == rev.tobytes()


def test_hla_cohort_samples_takes_a_config_per_sample(pkg, gpu_ctx):
    """two samples of one haplotype at 22x: with normalized_coverage 22 the absent-capable gene is hemizygous, with 11 it is not -- one shared
    config could not give both; each (sample, gene) equals the single-sample call with that sample's config"""
    from pb_starphase_amd import synth
    fx = synth.HlaFixture(max_alleles_per_gene=150, seed=4)
    db = fx.make_db(pkg, gpu_ctx)
    rng = np.random.default_rng(404)
    g = 0
    reads = []
    for _s in range(2):
        a = int(rng.choice(fx.full_length_alleles(g)))
        hap, st = fx.haplotype(g, a)
        reads.append(synth.simulate_reads(rng, hap, st, len(fx.dna[a]), 22, mean_len=7000, sd_len=1500, min_overlap=2500))
    cfgs = [[pkg.ffi.hla_call_config(absent_capable=True, normalized_coverage=cov)] for cov in (22.0, 11.0)]
    R = gpu_ctx.upload(reads[0] + reads[1])
    k1 = db.realign_reads(R)
    calls = db.diplotype_cohort_samples(2, [0] * len(reads[0]) + [1] * len(reads[1]), [g], R, k1, cfgs)
    for s in range(2):
        Rs = gpu_ctx.upload(reads[s])
        call, c1, c2, _is1 = db.diplotype_gene(g, Rs, db.realign_reads(Rs), cfg=cfgs[s][0])
        got, g1, g2 = calls[s][0]
        assert (got.allele1, got.allele2, got.is_hemizygous, got.is_dual, g1, g2) == (call.allele1, call.allele2, call.is_hemizygous, call.is_dual, c1, c2), s
    assert calls[0][0][0].is_hemizygous == 1 and calls[1][0][0].is_hemizygous == 0


def cyp_reads(pkg, sample):
    cfg, _gd = cr.load_db()
    s5 = cfg["cyp2d6_star5_del"]
    lo = min(min(cfg["cyp_coordinates"][k]["start"] for k in ("CYP2D6", "CYP2D7", "REP6", "REP7")), s5["start"] - 500)
    hi = max(max(cfg["cyp_coordinates"][k]["end"] for k in ("CYP2D6", "CYP2D7", "REP6", "REP7")), s5["end"] + 3000)
    return sorted(fetch_order(sample, [("chr22", lo, hi)], pkg.database), key=lambda x: x[1])


def test_cyp_cohort_mappings_equal_single_mappings(pkg, gpu_ctx, cohort):
    D = pkg.database
    s0 = cohort[0]
    dbf = D.Database(s0.db)
    w_chrom, _ws, _we = dbf.cyp_window()
    fasta = D.Fasta(s0.fasta)
    cdb = dbf.cyp_db(gpu_ctx, fasta.fetch(w_chrom, s0.locus.start, s0.locus.start + len(s0.locus.sequence)), s0.locus.start)
    sets = [gpu_ctx.upload([r[2] for r in cyp_reads(pkg, c)]) for c in cohort[:4]]
    got = D.cyp_diplotype_cohort_mappings(cdb, sets)
    for k, S in enumerate(sets):
        call, maps = D.cyp_diplotype_mappings(cdb, S)
        g_call, g_maps, rc = got[k]
        assert rc == 0 and (g_call.hap1, g_call.hap2, g_call.status) == (call.hap1, call.hap2, call.status), k
        assert g_maps == maps and len(maps) > 0, k


# ------------------------------------------------------------------ the command line
def test_cli_batch_writes_the_api_files(pkg, cohort, handle, tmp_path):
    D = pkg.database
    inputs = batch_inputs(cohort, tmp_path)[:5]
    (tmp_path / "corrupt.bam").write_bytes(b"not a BAM file")                       # exists (no NOINPUT), cannot be read: the call of that row fails
    inputs.append(dict(bams=[str(tmp_path / "corrupt.bam")], vcf=cohort[5].vcf))
    rows = []
    for i, kw in enumerate(inputs):
        rows.append("\t".join([str(tmp_path / f"calls{i}.json"), ",".join(kw.get("bams", [])), kw.get("vcf") or "-", kw.get("sample_name") or "-", "-",
                               str(tmp_path / f"calls{i}.tsv"), "-"]))
    (tmp_path / "samples.tsv").write_text("#output_calls\tbams\tvcf\tsample_name\tsv_vcf\tpharmcat_tsv\toutput_debug\n" + "\n".join(rows) + "\n")
    env = dict(os.environ, SP_K1_SLICE="16")                    # the child's K1 passes go through in slices
    p = subprocess.run([D.cli_path(), "diplotype-batch", "-d", cohort[0].db, "-r", cohort[0].fasta, "--manifest", str(tmp_path / "samples.tsv"),
                        "--max-group", "4", "-t", "4", "-v"], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 65, p.stderr[-2000:]
    assert "manifest row 6:" in p.stderr and "corrupt.bam" in p.stderr and "batch " in p.stderr
    assert not (tmp_path / "calls5.json").exists()
    want = handle.call_batch(inputs)
    for i in range(5):
        want[i].save(str(tmp_path / "api.json")); want[i].save_pharmcat_tsv(str(tmp_path / "api.tsv"))
        assert (tmp_path / f"calls{i}.json").read_bytes() == (tmp_path / "api.json").read_bytes(), i
        assert (tmp_path / f"calls{i}.tsv").read_bytes() == (tmp_path / "api.tsv").read_bytes(), i
    print("\n" + p.stderr.strip().splitlines()[-1])

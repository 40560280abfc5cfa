"""consensus_support.json in the whole-sample calls (sp_starphase_set_consensus_support; `--debug-consensus-support`; the `consensus_support` keyword of Starphase) on the
files of tests/test_gpu_diplotype_files.py.  The switch is off by default; off it changes nothing, on it adds the one file and changes no other byte.  The file's numbers
are held to the API: the step-by-step path on the same reads (sp_hla_realign_reads + sp_hla_diplotype_genes, then sp_hla_consensus_support) rendered through
sp_consensus_support_json must give the file's text."""
import json
import os
import subprocess

import pytest

from test_gpu_diplotype_files import Sample, fetch_order

pytestmark = pytest.mark.gpu
NAME = "consensus_support.json"


@pytest.fixture(scope="module")
def sample(pkg, tmp_path_factory):
    return Sample(tmp_path_factory.mktemp("sample"), pkg)


def files(folder):
    return {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))}


def run(pkg, sample, folder, on, touch=True, keyword=False, **kw):
    h = pkg.database.Starphase(sample.db, sample.fasta, debug_folder=str(folder), **(dict(consensus_support=True) if keyword else {}))
    if touch:
        h.set_consensus_support(on)
    res = h.call(**kw)
    out = (res.json(), res.pharmcat_tsv())
    h.close()
    return out


def expected_text(pkg, ctx, sample, hla_debug):
    """the file as the API gives it: the gene calls of the step-by-step path, their support tables, the typed alleles hla_debug.json names"""
    from pb_starphase_amd import synth
    D = pkg.database
    dbf, fasta = D.Database(sample.db), D.Fasta(sample.fasta)
    regions = dbf.hla_genes()
    hdb, _alleles = dbf.hla_db(ctx, [fasta.fetch(r["chrom"], r["start"] - 100, r["end"] + 100) for r in regions])
    met = fetch_order(sample, [(r["chrom"], r["start"], r["end"]) for r in regions], D)
    R = ctx.upload([x[2] for x in sorted(met, key=lambda x: x[1])])
    rec = hdb.realign_reads(R)
    calls, is1 = hdb.diplotype_genes(list(range(len(regions))), R, rec)
    entries, checked = [], 0
    for g, r in enumerate(regions):
        call, cons1, cons2 = calls[g]
        if call.status == 1:
            continue
        sup = hdb.consensus_support(g, R, rec, is1, cons1, cons2)
        strand = (lambda s: s) if r["is_forward_strand"] else synth.revcomp
        sides = []
        for k, cons in enumerate((cons1, cons2)):
            if not cons or (k == 1 and not call.is_dual):
                sides.append(None)
                continue
            typed = hla_debug["read_mapping_stats"][r["name"]]["consensus%d" % (k + 1)]["best_match_star"] or None
            sides.append((typed, strand(cons), sup[k][0], sup[k][1]))
            assert sup[k][1]["n_aligned"] >= 3 and sup[k][1]["median_depth"] >= 3
            checked += 1
        entries.append((r["name"], sides))
    R.close()
    hdb.close()
    assert checked >= 2
    return pkg.ffi.consensus_support_json(entries)


def test_switch_off_changes_nothing_and_on_adds_one_file(pkg, gpu_ctx, sample, tmp_path):
    kw = dict(bams=sample.bams, vcf=sample.vcf)
    never = run(pkg, sample, tmp_path / "never", False, touch=False, **kw)
    off = run(pkg, sample, tmp_path / "off", False, **kw)
    on = run(pkg, sample, tmp_path / "on", True, **kw)
    by_keyword = run(pkg, sample, tmp_path / "keyword", True, touch=False, keyword=True, **kw)
    f_never, f_off, f_on = files(tmp_path / "never"), files(tmp_path / "off"), files(tmp_path / "on")
    assert NAME not in f_never and f_off == f_never and off == never                      # calls JSON, TSV and every debug file: the same bytes
    assert on == never and by_keyword == never
    assert sorted(f_on) == sorted(list(f_never) + [NAME])
    assert {k: v for k, v in f_on.items() if k != NAME} == f_never
    assert files(tmp_path / "keyword") == f_on
    text = f_on[NAME].decode()
    got = json.loads(text)
    assert text == json.dumps(got, indent=2)
    assert text == expected_text(pkg, gpu_ctx, sample, json.loads(f_on["hla_debug.json"]))
    calls = json.loads(on[0])["gene_details"]
    for gene, per in got.items():
        haps = {h for d in calls[gene]["diplotypes"] for h in (d["hap1"], d["hap2"])}
        for rec in per.values():
            assert rec["n_members"] == rec["n_aligned"] + rec["n_unaligned"] and rec["n_contested"] == len(rec["contested"])
            assert rec["typed_allele"] is None or rec["typed_allele"].split("*", 1)[1] in {h.lstrip("*") for h in haps}
    # a sample without BAMs has no HLA lane: none of the lane's debug files; a BAM without HLA reads: the lane runs, no gene has a call, the file is an empty object
    run(pkg, sample, tmp_path / "vcf_only", True, vcf=sample.vcf2, sample_name=sample.sample_name)
    assert NAME not in files(tmp_path / "vcf_only") and "hla_debug.json" not in files(tmp_path / "vcf_only")
    import test_io
    empty = str(tmp_path / "no_reads.bam")
    test_io.write_bam(empty, sample.refs, [], 65280)
    run(pkg, sample, tmp_path / "no_reads", True, bams=[empty], vcf=sample.vcf)
    assert files(tmp_path / "no_reads")[NAME] == b"{}"


def test_switch_off_launches_nothing_and_takes_no_pool_memory(pkg, gpu_ctx, sample, tmp_path):
    """on a caller's context: warm calls with the switch off launch no pileup kernel and leave the context's pooled device memory as it was; the first call with the
    switch on launches it and only then takes the pass's buffers"""
    h = pkg.database.Starphase(sample.db, sample.fasta, ctx=gpu_ctx, debug_folder=str(tmp_path))
    kw = dict(bams=sample.bams, vcf=sample.vcf)
    h.call(**kw)
    before, launches = gpu_ctx.profile_get("pool:device"), gpu_ctx.profile_get("pileup")[1]
    h.set_consensus_support(False)
    h.call(**kw)
    assert gpu_ctx.profile_get("pool:device") == before and gpu_ctx.profile_get("pileup")[1] == launches and not os.path.exists(tmp_path / NAME)
    h.set_consensus_support(True)
    h.call(**kw)
    after = gpu_ctx.profile_get("pool:device")
    assert gpu_ctx.profile_get("pileup")[1] == launches + 1 and after[1] > before[1] and after[2] > before[2] and os.path.exists(tmp_path / NAME)
    h.close()


def test_batch_files_equal_the_single_calls(pkg, sample, tmp_path):
    inputs = [dict(bams=sample.bams, vcf=sample.vcf), dict(bams=[sample.hla_bam], vcf=sample.vcf2), dict(bams=sample.bams)]
    single = []
    for i, kw in enumerate(inputs):
        run(pkg, sample, tmp_path / f"single{i}", True, **kw)
        single.append(files(tmp_path / f"single{i}"))
    assert all(len(json.loads(s[NAME])) >= 1 for s in single)
    h = pkg.database.Starphase(sample.db, sample.fasta, consensus_support=True)
    for max_group in (1, 3):
        folders = [str(tmp_path / f"batch{max_group}_{i}") for i in range(len(inputs))]
        for f in folders:
            os.makedirs(f)
        got = h.call_batch(inputs, max_group=max_group, debug_folders=folders)
        assert not any(isinstance(g, Exception) for g in got)
        for i, f in enumerate(folders):
            assert files(f) == single[i], (max_group, i)
        # the middle sample without a debug folder: it gets no file, the others keep theirs
        folders = [str(tmp_path / f"part{max_group}_{i}") for i in range(len(inputs))]
        for f in folders:
            os.makedirs(f)
        got = h.call_batch(inputs, max_group=max_group, debug_folders=[folders[0], None, folders[2]])
        assert not any(isinstance(g, Exception) for g in got)
        assert os.listdir(folders[1]) == [] and files(folders[0]) == single[0] and files(folders[2]) == single[2]
    h.close()


def test_cli_flag(pkg, sample, tmp_path):
    D = pkg.database
    run(pkg, sample, tmp_path / "api", True, bams=sample.bams, vcf=sample.vcf)
    cmd = [D.cli_path(), "diplotype", "-d", sample.db, "-r", sample.fasta, "-c", sample.vcf, "-b", sample.bams[0], "--bam", sample.bams[1], "-o", str(tmp_path / "calls.json")]
    p = subprocess.run(cmd + ["--debug-consensus-support"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 64 and "--debug-consensus-support" in p.stderr and "--output-debug" in p.stderr
    p = subprocess.run(cmd + ["--debug-consensus-support", "--output-debug", str(tmp_path / "cli")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert os.path.exists(tmp_path / "cli" / NAME) and files(tmp_path / "cli") == files(tmp_path / "api")
    rows = [[str(tmp_path / "b0.json"), ",".join(sample.bams), sample.vcf, "-", "-", "-", str(tmp_path / "bdbg")]]
    man = tmp_path / "samples.tsv"
    man.write_text("\n".join("\t".join(r) for r in rows) + "\n")
    base = [D.cli_path(), "diplotype-batch", "-d", sample.db, "-r", sample.fasta, "--manifest", str(man)]
    p = subprocess.run(base + ["--debug-consensus-support"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert (tmp_path / "bdbg" / NAME).read_bytes() == (tmp_path / "api" / NAME).read_bytes()
    rows[0][6] = "-"
    man.write_text("\n".join("\t".join(r) for r in rows) + "\n")
    p = subprocess.run(base + ["--debug-consensus-support"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 64 and "--debug-consensus-support" in p.stderr
    for sub in ("diplotype", "diplotype-batch"):
        assert "--debug-consensus-support" in subprocess.run([D.cli_path(), sub, "--help"], capture_output=True, text=True).stdout

"""cyp2d6_consensus_support.json in the whole-sample calls (sp_starphase_set_cyp_consensus_support; `--debug-cyp2d6-support`; the `cyp_consensus_support` keyword of
Starphase) on the files of tests/test_gpu_diplotype_files.py.  The switch is its own: the HLA switch does not write this file.  Off it changes nothing, on it adds the
one file and changes no other byte.  The file's text is held to the step API: sp_cyp_diplotype_mappings on the same reads in QNAME order, sp_cyp_consensus_support on
what it returned, rendered through sp_cyp_support_json."""
import json
import os
import subprocess

import pytest

import cyp_cases_real as cr
from test_gpu_diplotype_files import Sample, fetch_order

pytestmark = pytest.mark.gpu
NAME = "cyp2d6_consensus_support.json"
CONS_CAP = 65536


@pytest.fixture(scope="module")
def sample(pkg, tmp_path_factory):
    return Sample(tmp_path_factory.mktemp("sample"), pkg)


def files(folder):
    return {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))}


def run(pkg, sample, folder, on, touch=True, keyword=False, **kw):
    h = pkg.database.Starphase(sample.db, sample.fasta, debug_folder=str(folder), **(dict(cyp_consensus_support=True) if keyword else {}))
    if touch:
        h.set_cyp_consensus_support(on)
    res = h.call(**kw)
    out = (res.json(), res.pharmcat_tsv())
    h.close()
    return out


@pytest.fixture(scope="module")
def expected_text(pkg, gpu_ctx, sample):
    """the file as the step API gives it"""
    D = pkg.database
    dbf, fasta = D.Database(sample.db), D.Fasta(sample.fasta)
    w_chrom, _ws, _we = dbf.cyp_window()
    cdb = dbf.cyp_db(gpu_ctx, fasta.fetch(w_chrom, sample.locus.start, sample.locus.start + len(sample.locus.sequence)), sample.locus.start)
    cfg, _gd = cr.load_db()
    keys = ("CYP2D6", "CYP2D7", "REP6", "REP7")
    s5 = cfg["cyp2d6_star5_del"]
    lo = min(min(cfg["cyp_coordinates"][k]["start"] for k in keys), s5["start"] - 500)
    hi = max(max(cfg["cyp_coordinates"][k]["end"] for k in keys), s5["end"] + 3000)
    reads = sorted(fetch_order(sample, [("chr22", lo, hi)], D), key=lambda x: x[1])
    R = gpu_ctx.upload([r[2] for r in reads])
    call, cons, mappings = D.cyp_call_with_consensus(cdb, R, CONS_CAP)
    assert call.status == 0 and len(mappings) > 0
    cols, sums = D.cyp_consensus_support(gpu_ctx, R, call, cons, CONS_CAP, mappings)
    assert max(s["median_depth"] for s in sums) >= 3 and sum(s["n_members"] for s in sums) == len(mappings)
    return D.cyp_support_json(call, [D.cyp_consensus_of(cons, CONS_CAP, h) for h in range(call.n_consensus)], cols, sums)


def test_switch_off_changes_nothing_and_on_adds_one_file(pkg, sample, expected_text, tmp_path):
    kw = dict(bams=sample.bams, vcf=sample.vcf)
    never = run(pkg, sample, tmp_path / "never", False, touch=False, **kw)
    off = run(pkg, sample, tmp_path / "off", False, **kw)
    on = run(pkg, sample, tmp_path / "on", True, **kw)
    by_keyword = run(pkg, sample, tmp_path / "keyword", True, touch=False, keyword=True, **kw)
    f_never, f_off, f_on = files(tmp_path / "never"), files(tmp_path / "off"), files(tmp_path / "on")
    assert sorted(f_never) == ["cyp2d6_alleles.json", "hla_debug.json"]                     # the listing as it was
    assert f_off == f_never and off == never                                                # calls JSON, TSV and every debug file: the same bytes
    assert on == never and by_keyword == never
    assert sorted(f_on) == sorted(list(f_never) + [NAME])
    assert {k: v for k, v in f_on.items() if k != NAME} == f_never
    assert files(tmp_path / "keyword") == f_on
    text = f_on[NAME].decode()
    assert text == expected_text
    got = json.loads(text)
    assert text == json.dumps(got, indent=2) and len(got) >= 2
    assert list(got) == sorted(got, key=lambda k: int(k.split("_", 1)[0]))                 # consensus order
    assert set(got) >= set(json.loads(f_on["cyp2d6_alleles.json"])["alleles"])              # the keys of cyp2d6_alleles.json
    for key, rec in got.items():
        assert rec["n_members"] == rec["n_aligned"] + rec["n_unaligned"] and rec["n_contested"] == len(rec["contested"]) and key.split("_", 1)[1] == rec["region_type"]
    # the HLA switch does not write this file, and this switch does not write the HLA file
    h = pkg.database.Starphase(sample.db, sample.fasta, debug_folder=str(tmp_path / "hla_switch"), consensus_support=True)
    h.call(**kw)
    h.close()
    assert sorted(files(tmp_path / "hla_switch")) == sorted(list(f_never) + ["consensus_support.json"])
    # a sample without CYP2D6 reads has no call: no file
    run(pkg, sample, tmp_path / "no_cyp", True, bams=[sample.hla_bam], vcf=sample.vcf)
    assert NAME not in files(tmp_path / "no_cyp")


def test_switch_off_launches_nothing(pkg, gpu_ctx, sample, tmp_path):
    """on a caller's context: a warm call with the switch off writes no file and leaves the context's pooled device memory as it was (the driver then hands the calls
    no consensus buffer and never reaches the pass: sp_diplotype.hip, cyp_group); the next call with the switch on writes the file"""
    h = pkg.database.Starphase(sample.db, sample.fasta, ctx=gpu_ctx, debug_folder=str(tmp_path))
    kw = dict(bams=sample.bams, vcf=sample.vcf)
    h.call(**kw)
    before = gpu_ctx.profile_get("pool:device")
    h.set_cyp_consensus_support(False)
    h.call(**kw)
    assert gpu_ctx.profile_get("pool:device") == before and not os.path.exists(tmp_path / NAME)
    h.set_cyp_consensus_support(True)
    h.call(**kw)
    assert os.path.exists(tmp_path / NAME)
    h.close()


def test_batch_files_equal_the_single_calls(pkg, sample, tmp_path):
    inputs = [dict(bams=sample.bams, vcf=sample.vcf), dict(bams=[sample.hla_bam], vcf=sample.vcf2), dict(bams=sample.bams)]
    single = []
    for i, kw in enumerate(inputs):
        run(pkg, sample, tmp_path / f"single{i}", True, **kw)
        single.append(files(tmp_path / f"single{i}"))
    assert NAME in single[0] and NAME not in single[1] and NAME in single[2]
    h = pkg.database.Starphase(sample.db, sample.fasta, cyp_consensus_support=True)
    for max_group in (1, 2):
        folders = [str(tmp_path / f"batch{max_group}_{i}") for i in range(len(inputs))]
        for f in folders:
            os.makedirs(f)
        got = h.call_batch(inputs, max_group=max_group, debug_folders=folders)
        assert not any(isinstance(g, Exception) for g in got)
        for i, f in enumerate(folders):
            assert files(f) == single[i], (max_group, i)
    # both samples with CYP2D6 reads in one group: one pass for two samples; then the first without a debug folder
    both = [inputs[0], inputs[2]]
    folders = [str(tmp_path / f"pair_{i}") for i in range(2)]
    for f in folders:
        os.makedirs(f)
    got = h.call_batch(both, max_group=2, debug_folders=folders)
    assert not any(isinstance(g, Exception) for g in got)
    assert files(folders[0]) == single[0] and files(folders[1]) == single[2]
    part = str(tmp_path / "part")
    os.makedirs(part)
    got = h.call_batch(both, max_group=2, debug_folders=[None, part])
    assert not any(isinstance(g, Exception) for g in got) and files(part) == single[2]
    h.close()


def test_cli_flag(pkg, sample, expected_text, tmp_path):
    D = pkg.database
    cmd = [D.cli_path(), "diplotype", "-d", sample.db, "-r", sample.fasta, "-c", sample.vcf, "-b", sample.bams[0], "--bam", sample.bams[1], "-o", str(tmp_path / "calls.json")]
    p = subprocess.run(cmd + ["--debug-cyp2d6-support"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 64 and "--debug-cyp2d6-support needs a debug folder (--output-debug <DIR>)" in p.stderr
    p = subprocess.run(cmd + ["--debug-cyp2d6-support", "--output-debug", str(tmp_path / "cli")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / "cli")) == ["cyp2d6_alleles.json", NAME, "hla_debug.json"]
    assert (tmp_path / "cli" / NAME).read_text() == expected_text
    rows = [[str(tmp_path / "b0.json"), ",".join(sample.bams), sample.vcf, "-", "-", "-", str(tmp_path / "bdbg")]]
    man = tmp_path / "samples.tsv"
    man.write_text("\n".join("\t".join(r) for r in rows) + "\n")
    base = [D.cli_path(), "diplotype-batch", "-d", sample.db, "-r", sample.fasta, "--manifest", str(man)]
    p = subprocess.run(base + ["--debug-cyp2d6-support"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert (tmp_path / "bdbg" / NAME).read_text() == expected_text
    rows[0][6] = "-"
    man.write_text("\n".join("\t".join(r) for r in rows) + "\n")
    p = subprocess.run(base + ["--debug-cyp2d6-support"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 64 and "--debug-cyp2d6-support" in p.stderr
    for sub in ("diplotype", "diplotype-batch"):
        assert "--debug-cyp2d6-support" in subprocess.run([D.cli_path(), sub, "--help"], capture_output=True, text=True).stdout

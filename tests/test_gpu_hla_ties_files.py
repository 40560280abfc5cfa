"""hla_ties.json in the whole-sample calls (sp_starphase_set_hla_ties; `--debug-hla-ties`; Starphase(hla_ties=True)): for each HLA consensus the alleles its call cannot
tell from the winner of the a = 5 scan -- on the files of tests/test_gpu_diplotype_files.py.  The switch is off by default; off it changes nothing, on it adds
hla_ties.json and changes no other byte.  The consensuses come from the step-by-step path of tests/test_gpu_hla_debug_mappings.py on the same reads, and the lists are
checked against m.ties[1] of a direct map_type_consensus(..., ties=True) on them."""
import json
import os
import subprocess

import pytest

from test_gpu_diplotype_files import Sample
from test_gpu_hla_debug_mappings import Steps, files

pytestmark = pytest.mark.gpu
NAME = "hla_ties.json"
CLASSES = ("distinct", "score_only", "equal", "beats_winner", "winner")


@pytest.fixture(scope="module")
def sample(pkg, tmp_path_factory):
    return Sample(tmp_path_factory.mktemp("sample"), pkg)


@pytest.fixture(scope="module")
def steps(pkg, gpu_ctx, sample):
    return Steps(pkg, gpu_ctx, sample)


def run(pkg, sample, folder, mode, mappings=False, **kw):
    """mode: "never" (a handle that was never told), "off", "on" (the setter; Starphase(hla_ties=True) is the batch test's)"""
    h = pkg.database.Starphase(sample.db, sample.fasta, debug_folder=str(folder))
    if mode in ("off", "on"):
        h.set_hla_ties(mode == "on")
    if mappings:
        h.set_hla_debug_mappings(True)
    res = h.call(**kw)
    out = (res.json(), res.pharmcat_tsv(), h.warnings())
    h.close()
    return out


def check_file(steps, text):
    doc = json.loads(text)
    assert text == json.dumps(doc, indent=2) and list(doc) == sorted(doc) == ["HLA-A", "HLA-B"]
    n_lists = 0
    for gene, per in doc.items():
        g = [r["name"] for r in steps.regions].index(gene)
        call = steps.calls[g][0]
        assert list(per) == (["consensus1", "consensus2"] if call.is_dual else ["consensus1"])
        for k, (who, rec) in enumerate(per.items()):
            assert list(rec) == ["typed_allele", "winner", "scan", "n_alleles", "counts", "equal", "score_only", "beats_winner"]
            m = steps.hdb.map_type_consensus(g, steps.calls[g][1 + k], ties=True)
            name = lambda a: gene + "*" + steps.alleles[int(a)][2]
            typed = call.typed2 if k else call.typed1
            assert rec["typed_allele"] == (name(typed) if typed >= 0 else None) and rec["winner"] == (name(m.best_mm2) if m.best_mm2 >= 0 else None)
            assert rec["scan"] == "mm2" and rec["n_alleles"] == len(m.alleles)
            assert rec["counts"] == dict(zip(CLASSES, (int(x) for x in m.tie_counts[1])))
            for c, key in ((2, "equal"), (1, "score_only"), (3, "beats_winner")):
                want = [name(a) for a, x in zip(m.alleles, m.ties[1]) if x == c]
                assert rec[key]["names"] == want[:256] and rec[key].get("more", 0) == max(0, len(want) - 256), (gene, who, key)
                assert ("more" in rec[key]) == (len(want) > 256)
                n_lists += 1
            print(gene, who, "typed", rec["typed_allele"], "winner", rec["winner"], rec["counts"])
    return n_lists


def test_switch_off_and_on(pkg, sample, steps, tmp_path):
    kw = dict(bams=sample.bams, vcf=sample.vcf)
    never = run(pkg, sample, tmp_path / "never", "never", **kw)
    off = run(pkg, sample, tmp_path / "off", "off", **kw)
    f_never, f_off = files(tmp_path / "never"), files(tmp_path / "off")
    assert sorted(f_never) == ["cyp2d6_alleles.json", "hla_debug.json"] and NAME not in f_off
    assert off[:2] == never[:2] and f_off == f_never
    on = run(pkg, sample, tmp_path / "on", "on", **kw)
    f_on = files(tmp_path / "on")
    assert sorted(f_on) == ["cyp2d6_alleles.json", "hla_debug.json", NAME]
    assert on == never                                         # calls JSON, PharmCAT TSV, warnings
    assert {k: v for k, v in f_on.items() if k != NAME} == f_never
    assert check_file(steps, f_on[NAME].decode()) >= 6
    # both switches: ONE map call serves both files, and each file is what its own switch writes
    both = run(pkg, sample, tmp_path / "both", "on", mappings=True, **kw)
    run(pkg, sample, tmp_path / "maps", "never", mappings=True, **kw)
    f_both, f_maps = files(tmp_path / "both"), files(tmp_path / "maps")
    assert both[:2] == never[:2] and f_both[NAME] == f_on[NAME] and {k: v for k, v in f_both.items() if k != NAME} == f_maps
    # a VCF-only call has no HLA pass: none of its debug files, this one included
    run(pkg, sample, tmp_path / "vcf_only", "on", vcf=sample.vcf2, sample_name=sample.sample_name)
    assert NAME not in files(tmp_path / "vcf_only")


def test_a_batch_writes_each_sample_the_file_of_its_single_call(pkg, sample, tmp_path):
    inputs = [dict(bams=sample.bams, vcf=sample.vcf), dict(bams=[sample.hla_bam], vcf=sample.vcf2)]
    single = []
    for i, kw in enumerate(inputs):
        run(pkg, sample, tmp_path / f"single{i}", "on", **kw)
        single.append(files(tmp_path / f"single{i}"))
    assert all(b'"names"' in s[NAME] for s in single)
    h = pkg.database.Starphase(sample.db, sample.fasta, hla_ties=True)
    folders = [str(tmp_path / f"batch{i}") for i in range(len(inputs))]
    for f in folders:
        os.makedirs(f)
    got = h.call_batch(inputs, debug_folders=folders)
    h.close()
    assert not any(isinstance(g, Exception) for g in got)
    for i, f in enumerate(folders):
        assert files(f) == single[i], i


def test_cli(pkg, sample, tmp_path):
    D = pkg.database
    run(pkg, sample, tmp_path / "api", "on", bams=sample.bams, vcf=sample.vcf)
    cmd = [D.cli_path(), "diplotype", "-d", sample.db, "-r", sample.fasta, "-c", sample.vcf, "-b", sample.bams[0], "--bam", sample.bams[1], "-o", str(tmp_path / "calls.json")]
    p = subprocess.run(cmd + ["--debug-hla-ties", "--output-debug", str(tmp_path / "cli")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert files(tmp_path / "cli") == files(tmp_path / "api")
    p = subprocess.run(cmd + ["--debug-hla-ties"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 64 and len(p.stderr.strip().splitlines()) == 1 and "--debug-hla-ties" in p.stderr
    rows = [[str(tmp_path / "b0.json"), ",".join(sample.bams), sample.vcf, "-", "-", "-", str(tmp_path / "bdbg")]]
    man = tmp_path / "samples.tsv"
    man.write_text("\n".join("\t".join(r) for r in rows) + "\n")
    p = subprocess.run([D.cli_path(), "diplotype-batch", "-d", sample.db, "-r", sample.fasta, "--manifest", str(man), "--debug-hla-ties"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert (tmp_path / "bdbg" / NAME).read_bytes() == (tmp_path / "api" / NAME).read_bytes()
    for sub in ("diplotype", "diplotype-batch"):
        assert "--debug-hla-ties" in subprocess.run([D.cli_path(), sub, "--help"], capture_output=True, text=True).stdout
    # what the command line refused before, it still refuses
    p = subprocess.run(cmd + ["--hla-revert-method"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 64 and "--hla-revert-method is not supported" in p.stderr

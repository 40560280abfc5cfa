"""cyp2d6_alleles.vcf.gz in the whole-sample calls (sp_starphase_set_cyp_vcf; `--debug-cyp2d6-vcf`; the `cyp_vcf` keyword of Starphase) on the files of
tests/test_gpu_diplotype_files.py: off it changes nothing, on it adds the one file and changes no other byte; the batch call's file equals the single call's; with
cyp2d6_consensus_support.json asked for as well both files equal their stand-alone versions."""
import gzip
import os
import subprocess

import pytest

from test_gpu_diplotype_files import Sample

pytestmark = pytest.mark.gpu
NAME = "cyp2d6_alleles.vcf.gz"
JSON = "cyp2d6_consensus_support.json"


@pytest.fixture(scope="module")
def sample(pkg, tmp_path_factory):
    return Sample(tmp_path_factory.mktemp("sample"), pkg)


def files(folder):
    return {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))}


def body(raw):
    """the text without the fileDate and command lines"""
    return [l for l in gzip.decompress(raw).decode().splitlines() if not l.startswith(("##fileDate=", "##pbstarphase_command="))]


def run(pkg, sample, folder, **switches):
    h = pkg.database.Starphase(sample.db, sample.fasta, debug_folder=str(folder), **switches)
    res = h.call(bams=sample.bams, vcf=sample.vcf)
    out = (res.json(), res.pharmcat_tsv())
    h.close()
    return out


@pytest.fixture(scope="module")
def singles(pkg, sample, tmp_path_factory):
    root = tmp_path_factory.mktemp("single")
    off = run(pkg, sample, root / "off")
    on = run(pkg, sample, root / "on", cyp_vcf=True)
    return dict(root=root, off=off, on=on, f_off=files(root / "off"), f_on=files(root / "on"))


def test_switch_off_changes_nothing_and_on_adds_one_file(singles):
    s = singles
    assert sorted(s["f_off"]) == ["cyp2d6_alleles.json", "hla_debug.json"]                  # the listing as it was: no file with the switch off
    assert s["on"] == s["off"]                                                              # calls JSON and TSV: the same bytes
    assert sorted(s["f_on"]) == sorted(list(s["f_off"]) + [NAME])
    assert {k: v for k, v in s["f_on"].items() if k != NAME} == s["f_off"]
    raw = s["f_on"][NAME]
    assert raw.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    lines = gzip.decompress(raw).decode().splitlines()
    assert lines[0] == "##fileformat=VCFv4.2" and any(l.startswith("##FORMAT=<ID=SR,") for l in lines) and any(l.startswith("##FORMAT=<ID=CR,") for l in lines)
    records = [l.split("\t") for l in lines if not l.startswith("#")]
    head = [l for l in lines if l.startswith("#CHROM")][0].split("\t")
    assert len(head) > 9 and records and all(r[8] == "GT:SR:CR" and len(r) == len(head) for r in records)
    cells = [c.split(":") for r in records for c in r[9:]]
    assert all(len(c) == 3 for c in cells) and any(c[1] != "." and int(c[1]) >= 3 for c in cells)
    assert all(c[1] == "." or int(c[2]) <= int(c[1]) for c in cells)


def test_batch_files_equal_the_single_call(pkg, sample, singles, tmp_path):
    h = pkg.database.Starphase(sample.db, sample.fasta, cyp_vcf=True)
    inputs = [dict(bams=sample.bams, vcf=sample.vcf), dict(bams=[sample.hla_bam], vcf=sample.vcf2), dict(bams=sample.bams)]
    folders = [str(tmp_path / f"b{i}") for i in range(3)]
    for f in folders:
        os.makedirs(f)
    got = h.call_batch(inputs, max_group=3, debug_folders=folders)
    assert not any(isinstance(g, Exception) for g in got)
    f0, f1, f2 = (files(f) for f in folders)
    assert NAME not in f1                                                                   # no CYP2D6 reads: no call, no file
    assert body(f0[NAME]) == body(singles["f_on"][NAME]) == body(f2[NAME])
    assert {k: v for k, v in f0.items() if k != NAME} == singles["f_off"]
    part = str(tmp_path / "part")
    os.makedirs(part)
    got = h.call_batch([inputs[0], inputs[2]], max_group=2, debug_folders=[None, part])      # no debug folder: no file
    assert not any(isinstance(g, Exception) for g in got) and body(files(part)[NAME]) == body(singles["f_on"][NAME])
    h.close()


def test_with_the_support_file_asked_for_as_well_both_equal_their_stand_alone_versions(pkg, sample, singles, tmp_path):
    """(that ONE member pass serves both is counted at the step API: tests/test_gpu_cyp_variant_vcf.py -- the whole-sample call runs its CYP2D6 lane on a context of
    its own, whose launch counts no caller sees)"""
    run(pkg, sample, tmp_path / "json_alone", cyp_consensus_support=True)
    run(pkg, sample, tmp_path / "both", cyp_consensus_support=True, cyp_vcf=True)
    both = files(tmp_path / "both")
    assert both[JSON] == files(tmp_path / "json_alone")[JSON] and body(both[NAME]) == body(singles["f_on"][NAME])
    assert {k: v for k, v in both.items() if k not in (NAME, JSON)} == singles["f_off"]


def test_cli_flag(pkg, sample, singles, tmp_path):
    D = pkg.database
    cmd = [D.cli_path(), "diplotype", "-d", sample.db, "-r", sample.fasta, "-c", sample.vcf, "-b", sample.bams[0], "--bam", sample.bams[1], "-o", str(tmp_path / "calls.json")]
    p = subprocess.run(cmd + ["--debug-cyp2d6-vcf"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 64 and "--debug-cyp2d6-vcf needs a debug folder (--output-debug <DIR>)" in p.stderr
    p = subprocess.run(cmd + ["--debug-cyp2d6-vcf", "--output-debug", str(tmp_path / "cli")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / "cli")) == sorted(["cyp2d6_alleles.json", NAME, "hla_debug.json"])
    assert body(open(tmp_path / "cli" / NAME, "rb").read()) == body(singles["f_on"][NAME])
    for sub in ("diplotype", "diplotype-batch"):
        assert "--debug-cyp2d6-vcf" in subprocess.run([D.cli_path(), sub, "--help"], capture_output=True, text=True).stdout

"""cyp2d6_alternatives.json in the whole-sample calls (sp_starphase_set_cyp_alternatives; `--debug-cyp2d6-alternatives`; the `cyp_alternatives` keyword of
Starphase) on the files of tests/test_gpu_diplotype_files.py: off there is no file, on it adds the one file and changes no other byte; entry 0 is the call; the
batch call's file equals the single call's."""
import json
import os
import subprocess

import pytest

from test_gpu_cyp_vcf_files import files, run, sample  # noqa: F401  (sample: the module-scoped fixture of that file)

pytestmark = pytest.mark.gpu
NAME = "cyp2d6_alternatives.json"


@pytest.fixture(scope="module")
def singles(pkg, sample, tmp_path_factory):
    root = tmp_path_factory.mktemp("single_alt")
    off = run(pkg, sample, root / "off")
    on = run(pkg, sample, root / "on", cyp_alternatives=True)
    return dict(root=root, off=off, on=on, f_off=files(root / "off"), f_on=files(root / "on"))


def test_switch_off_no_file_and_on_adds_one_file(singles):
    s = singles
    assert sorted(s["f_off"]) == ["cyp2d6_alleles.json", "hla_debug.json"]                  # the listing as it was: no file with the switch off
    assert s["on"] == s["off"]                                                              # calls JSON and TSV: the same bytes
    assert sorted(s["f_on"]) == sorted(list(s["f_off"]) + [NAME])
    assert {k: v for k, v in s["f_on"].items() if k != NAME} == s["f_off"]
    doc = json.loads(s["f_on"][NAME])
    assert list(doc) == ["n_possible_chains", "alternatives"]                               # n_pairs_scored differs from run to run: not in the file
    alts = doc["alternatives"]
    assert 1 <= len(alts) <= 10 and [a["rank"] for a in alts] == list(range(1, len(alts) + 1))
    calls = json.loads(s["on"][0])
    cyp = calls["gene_details"]["CYP2D6"]["diplotypes"][0]["diplotype"]
    assert alts[0]["diplotype"] == cyp and alts[0]["delta_to_best"] == 0.0
    scores = [a["score"] for a in alts]
    assert scores == sorted(scores) and all(abs(a["delta_to_best"] - (a["score"] - scores[0])) < 1e-9 for a in alts)
    for a in alts:
        assert len(a["chains"]) == 2 and a["coverage"] and all(c["copies"] > 0 for c in a["coverage"])
        assert abs(a["score"] - (a["ln_ed_penalty"] + a["mn_llh_penalty"] + a["allele_expected_penalty"] + a["unexpected_chain_penalty"] + a["inferred_chain_penalty"])) < 1e-9


def test_batch_files_equal_the_single_call(pkg, sample, singles, tmp_path):
    h = pkg.database.Starphase(sample.db, sample.fasta, cyp_alternatives=True)
    inputs = [dict(bams=sample.bams, vcf=sample.vcf), dict(bams=[sample.hla_bam], vcf=sample.vcf2), dict(bams=sample.bams)]
    folders = [str(tmp_path / f"b{i}") for i in range(3)]
    for f in folders:
        os.makedirs(f)
    got = h.call_batch(inputs, max_group=3, debug_folders=folders)
    assert not any(isinstance(g, Exception) for g in got)
    f0, f1, f2 = (files(f) for f in folders)
    assert NAME not in f1                                                                   # no CYP2D6 reads: no call, no file
    assert f0[NAME] == singles["f_on"][NAME] == f2[NAME]                                    # two samples of one cohort call: each the bytes of its single call
    assert {k: v for k, v in f0.items() if k != NAME} == singles["f_off"]
    part = str(tmp_path / "part")
    os.makedirs(part)
    got = h.call_batch([inputs[0], inputs[2]], max_group=2, debug_folders=[None, part])      # no debug folder: no file
    assert not any(isinstance(g, Exception) for g in got) and files(part)[NAME] == singles["f_on"][NAME]
    h.close()


def test_cli_flag(pkg, sample, singles, tmp_path):
    D = pkg.database
    cmd = [D.cli_path(), "diplotype", "-d", sample.db, "-r", sample.fasta, "-c", sample.vcf, "-b", sample.bams[0], "--bam", sample.bams[1], "-o", str(tmp_path / "calls.json")]
    p = subprocess.run(cmd + ["--debug-cyp2d6-alternatives"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 64 and "--debug-cyp2d6-alternatives needs a debug folder (--output-debug <DIR>)" in p.stderr
    p = subprocess.run(cmd + ["--debug-cyp2d6-alternatives", "--output-debug", str(tmp_path / "cli")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / "cli")) == sorted(["cyp2d6_alleles.json", NAME, "hla_debug.json"])
    assert open(tmp_path / "cli" / NAME, "rb").read() == singles["f_on"][NAME]
    for sub in ("diplotype", "diplotype-batch"):
        assert "--debug-cyp2d6-alternatives" in subprocess.run([D.cli_path(), sub, "--help"], capture_output=True, text=True).stdout
    p = subprocess.run([D.cli_path(), "diplotype-batch", "--debug-cyp2d6-alternatives"], capture_output=True, text=True)    # accepted: only the required ones are missed
    assert p.returncode == 2 and "unexpected argument" not in p.stderr and "required arguments were not provided" in p.stderr

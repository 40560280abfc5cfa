"""variant_alternatives.json in the whole-sample calls (sp_starphase_set_variant_alternatives; `--debug-variant-alternatives`; the `variant_alternatives` keyword of
Starphase) on the files of tests/test_gpu_diplotype_files.py: off there is no file, on it adds the one file and changes no other byte; the first called entry of
every gene is the call; the batch call's file equals the single call's."""
import json
import os
import subprocess

import pytest

from test_gpu_cyp_vcf_files import files, run, sample  # noqa: F401  (sample: the module-scoped fixture of that file)

pytestmark = pytest.mark.gpu
NAME = "variant_alternatives.json"
FIELDS = ["core_missing", "core_unexpected", "sub_missing", "sub_unexpected"]


@pytest.fixture(scope="module")
def singles(pkg, sample, tmp_path_factory):
    root = tmp_path_factory.mktemp("single_valt")
    off = run(pkg, sample, root / "off")
    on = run(pkg, sample, root / "on", variant_alternatives=True)
    plain = run(pkg, sample, root / "plain", variant_alternatives=False)
    return dict(root=root, off=off, on=on, plain=plain, f_off=files(root / "off"), f_on=files(root / "on"), f_plain=files(root / "plain"))


def test_switch_off_no_file_and_on_adds_one_file(singles):
    s = singles
    assert NAME not in s["f_off"] and s["f_off"] == s["f_plain"] and s["off"] == s["plain"]      # no mention of the switch == switch off
    assert s["on"] == s["off"]                                                              # calls JSON and TSV: the same bytes
    assert sorted(s["f_on"]) == sorted(list(s["f_off"]) + [NAME])
    assert {k: v for k, v in s["f_on"].items() if k != NAME} == s["f_off"]


def test_the_file_agrees_with_the_calls(singles):
    doc = json.loads(singles["f_on"][NAME])
    details = json.loads(singles["on"][0])["gene_details"]
    solved = [g for g, d in details.items() if d["variant_details"] is not None and d["mapping_details"] is None and d["multi_mapping_details"] is None and g in doc]
    assert list(doc) == sorted(doc) and len(doc) >= 1 and solved == list(doc)
    # every variant gene of the sample is in the file, but for those answered without a solve (no variants in the database)
    for g, d in details.items():
        if g not in doc and d["mapping_details"] is None and d["multi_mapping_details"] is None:
            assert not d["variant_details"] and d["inexact_diplotypes"] is None
    checked_exact = checked_inexact = 0
    for g, e in doc.items():
        assert list(e) == ["n_combinations", "n_candidates", "best_score", "alternatives"]
        alts = e["alternatives"]
        assert len(alts) == min(10, e["n_candidates"]) and [a["rank"] for a in alts] == list(range(1, len(alts) + 1))
        keys = [[a["score"][f] for f in FIELDS] + [a["combination"]] for a in alts]
        assert keys == sorted(keys)
        d = details[g]
        called = [a for a in alts if a["called"]]
        if not called:
            assert [x["diplotype"] for x in d["diplotypes"]] == ["NO_MATCH/NO_MATCH"] or not alts
            continue
        first = called[0]
        assert first["score"] == alts[0]["score"] == e["best_score"] and not first["shadowed"]
        if d["inexact_diplotypes"] is None:
            assert first["diplotype"] == d["diplotypes"][0]["diplotype"] and set(first["score"].values()) == {0}
            checked_exact += 1
            continue
        assert first["diplotype"] == d["diplotypes"][0]["diplotype"]
        for key, hap in (("haplotype_1", "hap1"), ("haplotype_2", "hap2")):
            x = d["inexact_diplotypes"][0][key]
            assert x["base_haplotype"] == first[hap]["haplotype"]
            for state, name in (("Missing", "missing"), ("Unexpected", "unexpected")):
                assert sorted(r["label"] for r in x["variant_relationships"] if r["variant_state"] == state) == sorted(set(first[hap][name]))
        checked_inexact += 1
    assert checked_exact + checked_inexact >= 1


def test_batch_files_equal_the_single_call(pkg, sample, singles, tmp_path):
    h = pkg.database.Starphase(sample.db, sample.fasta, variant_alternatives=True)
    inputs = [dict(bams=sample.bams, vcf=sample.vcf), dict(bams=[sample.hla_bam], vcf=sample.vcf2), dict(bams=sample.bams)]
    folders = [str(tmp_path / f"b{i}") for i in range(3)]
    for f in folders:
        os.makedirs(f)
    got = h.call_batch(inputs, max_group=3, debug_folders=folders)
    assert not any(isinstance(g, Exception) for g in got)
    f0, f1, f2 = (files(f) for f in folders)
    assert NAME not in f2                                                                   # no VCF: no variant genes, no file
    assert f0[NAME] == singles["f_on"][NAME] and NAME in f1 and json.loads(f1[NAME])
    assert {k: v for k, v in f0.items() if k != NAME} == singles["f_off"]
    part = str(tmp_path / "part")
    os.makedirs(part)
    got = h.call_batch([inputs[1], inputs[0]], max_group=2, debug_folders=[None, part])     # no debug folder: no file; the other sample's bytes do not move
    assert not any(isinstance(g, Exception) for g in got) and files(part)[NAME] == singles["f_on"][NAME]
    h.close()


def test_cli_flag(pkg, sample, singles, tmp_path):
    D = pkg.database
    cmd = [D.cli_path(), "diplotype", "-d", sample.db, "-r", sample.fasta, "-c", sample.vcf, "-b", sample.bams[0], "--bam", sample.bams[1], "-o", str(tmp_path / "calls.json")]
    p = subprocess.run(cmd + ["--debug-variant-alternatives"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 64 and "--debug-variant-alternatives needs a debug folder (--output-debug <DIR>)" in p.stderr
    p = subprocess.run(cmd + ["--debug-variant-alternatives", "--output-debug", str(tmp_path / "cli")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / "cli")) == sorted(list(singles["f_off"]) + [NAME])
    assert open(tmp_path / "cli" / NAME, "rb").read() == singles["f_on"][NAME]
    for sub in ("diplotype", "diplotype-batch"):
        assert "--debug-variant-alternatives" in subprocess.run([D.cli_path(), sub, "--help"], capture_output=True, text=True).stdout

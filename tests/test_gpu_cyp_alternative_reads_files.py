"""cyp2d6_alternative_reads.json in the whole-sample calls (sp_starphase_set_cyp_alternative_reads; `--debug-cyp2d6-alternative-reads`; the `cyp_alternative_reads`
keyword of Starphase) on the files of tests/test_gpu_diplotype_files.py: off (a handle that saw the switch and one that never did) every file is the same bytes, on
it adds the one file and changes no other byte; the reads are named by QNAMEs of the fixture BAMs; rank 1 agrees with cyp2d6_alternatives.json; the CLI, the keyword
and a batch give the same bytes.

The fixture sample (*4/*4) is clean: under all ten pairs every read is neutral and the file lists none.  So the names are checked on a second sample, `het`: the
same database and reference with reads of *1.001/*2.001, whose runners-up leave reads unmet.  Its QNAMEs are scrambled against the BAM order, and what the file
must list is worked out from the calls JSON alone: multi_mapping_details gives every read with one observed chain its chain, by QNAME, and such a read is
unsupported under a pair exactly when that chain is no run of consecutive regions of either chain of the pair."""
import json
import os
import subprocess

import pytest

from test_gpu_cyp_vcf_files import files, run, sample  # noqa: F401  (sample: the module-scoped fixture of that file)

pytestmark = pytest.mark.gpu
NAME = "cyp2d6_alternative_reads.json"
ALTS = "cyp2d6_alternatives.json"


@pytest.fixture(scope="module")
def singles(pkg, sample, tmp_path_factory):
    root = tmp_path_factory.mktemp("single_alt_reads")
    never = run(pkg, sample, root / "never")
    h = pkg.database.Starphase(sample.db, sample.fasta, debug_folder=str(root / "off"), cyp_alternative_reads=True)
    h.set_cyp_alternative_reads(False)                                                          # a handle that saw the switch, and has it off
    res = h.call(bams=sample.bams, vcf=sample.vcf)
    off = (res.json(), res.pharmcat_tsv())
    h.close()
    on = run(pkg, sample, root / "on", cyp_alternative_reads=True)
    both = run(pkg, sample, root / "both", cyp_alternative_reads=True, cyp_alternatives=True)
    alts = run(pkg, sample, root / "alts", cyp_alternatives=True)
    return dict(never=never, off=off, on=on, both=both, alts=alts, **{"f_" + k: files(root / k) for k in ("never", "off", "on", "both", "alts")})


@pytest.fixture(scope="module")
def het(pkg, sample, tmp_path_factory):
    """the sample's database and reference with 120 reads of *1.001/*2.001 in one BAM; QNAME order is neither the order the reads were drawn in nor the BAM's"""
    import cyp_cases_real as cr
    import numpy as np
    import test_io
    root = tmp_path_factory.mktemp("het_alt_reads")
    _name, haps, _truth = cr.scenarios(sample.locus)[0]
    rng = np.random.default_rng(100)
    d6 = cr.load_db()[0]["cyp_coordinates"]["CYP2D6"]
    recs = [(1, d6["start"] + int(rng.integers(-8000, 2000)), "m84/%04d/ccs" % ((i * 7919 + 13) % 10000), 0, 60, [("M", len(q))], q)
            for i, q in enumerate(sample.locus.sample(rng, haps, 120, lo=8000, hi=16000))]
    bam = str(root / "het.bam")
    test_io.write_bam(bam, sample.refs, sorted(recs, key=lambda r: (r[0], r[1], r[2])), 65280)
    h = pkg.database.Starphase(sample.db, sample.fasta, debug_folder=str(root / "debug"), cyp_alternative_reads=True)
    calls = json.loads(h.call(bams=[bam]).json())
    h.close()
    return dict(qnames={r[2] for r in recs}, calls=calls, doc=json.loads(files(root / "debug")[NAME]))


def is_run(hay, needle):
    return any(hay[s:s + len(needle)] == needle for s in range(len(hay) - len(needle) + 1))


def test_the_listed_reads_are_the_expected_qnames(het):
    """the map from the problem's read to the sample's QNAME, through the lane: the unsupported reads of every pair, by name, against the calls JSON"""
    cyp = het["calls"]["gene_details"]["CYP2D6"]
    observed = {}                                                            # QNAME -> its one observed chain (the entries of a read come in chain order)
    for m in cyp["multi_mapping_details"]:
        observed.setdefault(m["read_qname"], []).append(m["consensus_id"])
    assert len(observed) > 60 and set(observed) <= het["qnames"]
    alts = het["doc"]["alternatives"]
    assert alts[0]["diplotype"] == cyp["diplotypes"][0]["diplotype"] and len(alts) == 10
    named = {r["read"] for a in alts for r in a["reads"]}
    assert named and named <= het["qnames"]
    checked = 0
    for a in alts:
        pair = [[int(x.split("_")[0]) for x in c] for c in a["chains"]]
        want = {q for q, ch in observed.items() if not (is_run(pair[0], ch) or is_run(pair[1], ch))}
        got = {r["read"] for r in a["reads"] if not r["supported"]}
        assert got & set(observed) == want, (a["rank"], sorted(got & set(observed)), sorted(want))
        assert a["unmet_observations"] == len(got) and sum(r["excess_ed"] for r in a["reads"]) == a["edit_distance"]
        checked += len(want)
        hap = {1: pair[a["hap1_chain"] - 1], 2: pair[2 - a["hap1_chain"]]}
        for r in a["reads"]:
            assert all(p.split("@")[0] in ("hap1", "hap2") for p in r["placements"])
            for p in r["placements"]:                                        # a placement lies on its chain
                assert int(p.split("@")[1]) < len(hap[int(p[3])])
    assert checked >= 10 and any(a["unmet_observations"] for a in alts[1:])
    first = {r["read"]: r["excess_ed"] for r in alts[0]["reads"]}
    for a in alts[1:]:
        assert a["reads"] and all(r["delta_to_best"] == r["excess_ed"] - first.get(r["read"], 0) for r in a["reads"])
        assert a["reads_decided_for"] == sum(1 for r in a["reads"] if r["delta_to_best"] > 0) > 0
        assert a["reads_decided_against"] == sum(1 for r in a["reads"] if r["delta_to_best"] < 0)


def test_switch_off_is_the_same_bytes_and_on_adds_one_file(singles):
    s = singles
    assert sorted(s["f_never"]) == ["cyp2d6_alleles.json", "hla_debug.json"]
    assert s["f_off"] == s["f_never"] and s["off"] == s["never"]
    assert s["on"] == s["never"]                                                                # calls JSON and TSV: the same bytes
    assert sorted(s["f_on"]) == sorted(list(s["f_never"]) + [NAME])
    assert {k: v for k, v in s["f_on"].items() if k != NAME} == s["f_never"]


def test_both_switches_one_search_two_files(singles):
    s = singles
    assert sorted(s["f_both"]) == sorted(list(s["f_never"]) + [NAME, ALTS])
    assert s["f_both"][NAME] == s["f_on"][NAME] and s["f_both"][ALTS] == s["f_alts"][ALTS]      # each as it is alone
    reads, alts = json.loads(s["f_both"][NAME]), json.loads(s["f_both"][ALTS])
    assert len(reads["alternatives"]) == len(alts["alternatives"])
    for a, b in zip(reads["alternatives"], alts["alternatives"]):
        assert (a["rank"], a["diplotype"], a["chains"], a["edit_distance"], a["unmet_observations"]) == \
               (b["rank"], b["diplotype"], b["chains"], b["edit_distance"], b["unmet_observations"])


def test_the_content_of_the_file(pkg, sample, singles):
    doc = json.loads(singles["f_on"][NAME])
    assert list(doc) == ["observed", "alternatives"]
    qnames = {r[2] for part in sample.recs_by_file for r in part if r[0] == 1}              # the QNAMEs of the chr22 records of the two BAMs
    alts = doc["alternatives"]
    assert 1 <= len(alts) <= 10 and [a["rank"] for a in alts] == list(range(1, len(alts) + 1))
    calls = json.loads(singles["on"][0])
    assert alts[0]["diplotype"] == calls["gene_details"]["CYP2D6"]["diplotypes"][0]["diplotype"]
    named = {r["read"] for a in alts for r in a["reads"]}
    assert not any(n.startswith("read ") for n in named) and named <= qnames, sorted(named - qnames)[:3]
    # (this sample's reads fit the call and its runners-up alike and none is listed: the names are held to the reads on `het`, above)
    assert "reads_decided_for" not in alts[0]
    for a in alts:
        assert a["hap1_chain"] in (1, 2) and len(a["chains"]) == 2
        assert sum(r["excess_ed"] for r in a["reads"]) == a["edit_distance"]                   # a neutral read has no excess
        assert sum(1 for r in a["reads"] if not r["supported"]) == a["unmet_observations"]
        for r in a["reads"]:
            assert all(p.split("@")[0] in ("hap1", "hap2") and p.split("@")[1].isdigit() for p in r["placements"])
    first = {r["read"]: r["excess_ed"] for r in alts[0]["reads"]}
    for a in alts[1:]:
        assert all(r["delta_to_best"] == r["excess_ed"] - first.get(r["read"], 0) for r in a["reads"])
        assert a["reads_decided_for"] == sum(1 for r in a["reads"] if r["delta_to_best"] > 0)
        assert a["reads_decided_against"] == sum(1 for r in a["reads"] if r["delta_to_best"] < 0)
    obs = doc["observed"]
    assert obs["chains"] and obs["regions"] and all(c["reads"] > 0 for c in obs["chains"])
    assert abs(sum(len(c["chain"]) * c["reads"] for c in obs["chains"]) - sum(r["reads"] for r in obs["regions"])) < 1e-6


def test_batch_files_equal_the_single_call(pkg, sample, singles, tmp_path):
    h = pkg.database.Starphase(sample.db, sample.fasta, cyp_alternative_reads=True)
    inputs = [dict(bams=sample.bams, vcf=sample.vcf), dict(bams=sample.bams)]
    folders = [str(tmp_path / f"b{i}") for i in range(2)]
    for f in folders:
        os.makedirs(f)
    got = h.call_batch(inputs, max_group=2, debug_folders=folders)
    assert not any(isinstance(g, Exception) for g in got)
    f0, f1 = (files(f) for f in folders)
    assert f0[NAME] == singles["f_on"][NAME] == f1[NAME]                                       # two samples of one cohort call: each the bytes of its single call
    assert {k: v for k, v in f0.items() if k != NAME} == singles["f_never"]
    h.close()


def test_cli_flag(pkg, sample, singles, tmp_path):
    D = pkg.database
    cmd = [D.cli_path(), "diplotype", "-d", sample.db, "-r", sample.fasta, "-c", sample.vcf, "-b", sample.bams[0], "--bam", sample.bams[1], "-o", str(tmp_path / "calls.json")]
    p = subprocess.run(cmd + ["--debug-cyp2d6-alternative-reads"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 64 and "--debug-cyp2d6-alternative-reads needs a debug folder (--output-debug <DIR>)" in p.stderr
    p = subprocess.run(cmd + ["--debug-cyp2d6-alternative-reads", "--output-debug", str(tmp_path / "cli")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / "cli")) == sorted(["cyp2d6_alleles.json", NAME, "hla_debug.json"])
    assert open(tmp_path / "cli" / NAME, "rb").read() == singles["f_on"][NAME]
    for sub in ("diplotype", "diplotype-batch"):
        assert "--debug-cyp2d6-alternative-reads" in subprocess.run([D.cli_path(), sub, "--help"], capture_output=True, text=True).stdout
    p = subprocess.run([D.cli_path(), "diplotype-batch", "--debug-cyp2d6-alternative-reads"], capture_output=True, text=True)    # accepted: only the required ones are missed
    assert p.returncode == 2 and "unexpected argument" not in p.stderr and "required arguments were not provided" in p.stderr

"""read_debug.json of the whole-sample calls (sp_starphase_set_read_debug; `--debug-reads`): per gene and QNAME the accepted allele of every realigned HLA read and
its mapping with CIGAR and MD -- on the files of tests/test_gpu_diplotype_files.py.  The switch is off by default and changes no other output."""
import json
import os
import re
import subprocess

import pytest

import affine_traceback_ref as ar
from test_gpu_diplotype_files import Sample

pytestmark = pytest.mark.gpu

LISTING = ["cyp2d6_alleles.json", "hla_debug.json", "read_debug.json"]


@pytest.fixture(scope="module")
def sample(pkg, tmp_path_factory):
    return Sample(tmp_path_factory.mktemp("sample"), pkg)


def run(pkg, sample, folder, on, **kw):
    h = pkg.database.Starphase(sample.db, sample.fasta, debug_folder=str(folder))
    if on:
        h.set_read_debug(True)
    res = h.call(**kw)
    out = (res.json(), res.pharmcat_tsv(), h.timing())
    h.close()
    return out


def ops_of(cigar, md):
    """the '=' / 'X' / 'I' / 'D' ops a (CIGAR string, MD tag) pair spells"""
    cols = []                                                # the target's columns: '=', 'X' or 'D'
    for num, dele, mis in re.findall(r"(\d+)|\^([ACGTN]+)|([ACGTN])", md):
        cols += ["="] * int(num) if num else (["D"] * len(dele) if dele else ["X"])
    steps, k = [], 0
    for n, op in [(int(n), op) for n, op in re.findall(r"(\d+)([MID])", cigar)]:
        if op == "I":
            steps += [1] * n
            continue
        part = cols[k:k + n]; k += n
        assert len(part) == n and all((c == "D") == (op == "D") for c in part), (cigar, md)
        steps += [2 if c == "D" else (7 if c == "=" else 8) for c in part]
    assert k == len(cols)
    ops = []
    for s in steps:
        if ops and ops[-1][1] == s:
            ops[-1] = (ops[-1][0] + 1, s)
        else:
            ops.append((1, s))
    return ops


def check_mapping(dm, read, allele):
    """the invariants of a CIGAR of the affine DP (affine_traceback_ref.check_ops) for a dna_mapping, whose spans the file gives by their lengths only: the one placement
    of the first run of matches that makes every column true"""
    assert dm["query_len"] == len(read) and dm["target_len"] == len(allele)
    ops = ops_of(dm["cigar"], dm["md"])
    t_span = sum(n for n, op in ops if op in (7, 8, 2)); q_span = sum(n for n, op in ops if op in (7, 8, 1))
    assert t_span == dm["target_len"] - dm["target_unmapped"] and q_span == dm["query_len"] - dm["query_unmapped"]
    assert dm["match_len"] == sum(n for n, op in ops if op == 7)
    assert ops[0][1] == 7 and ops[-1][1] == 7                   # a local alignment begins and ends with matches
    good = []
    for qs in range(dm["query_unmapped"] + 1):
        head = read[qs:qs + ops[0][0]]
        ts = allele.find(head, 0, dm["target_unmapped"] + ops[0][0])
        while ts >= 0:
            try:
                nm, _score = ar.check_ops(ops, allele, read, ts, ts + t_span, qs, qs + q_span)
                good.append((ts, qs, nm))
            except AssertionError:
                pass
            ts = allele.find(head, ts + 1, dm["target_unmapped"] + ops[0][0])
    assert good and all(nm == dm["nm"] for _t, _q, nm in good), (dm["cigar"][:80], good[:3])


def test_read_debug_of_a_sample(pkg, sample, tmp_path):
    on_dir, off_dir = tmp_path / "on", tmp_path / "off"
    kw = dict(bams=sample.bams, vcf=sample.vcf)
    js_off, tsv_off, t_off = run(pkg, sample, off_dir, False, **kw)
    js_on, tsv_on, t_on = run(pkg, sample, on_dir, True, **kw)
    print("\nhla_ms with the switch off / on:", round(t_off["hla_ms"], 2), "/", round(t_on["hla_ms"], 2))
    assert sorted(os.listdir(on_dir)) == LISTING and sorted(os.listdir(off_dir)) == LISTING[:2]
    # every other output is the same bytes
    assert (js_on, tsv_on) == (js_off, tsv_off)
    for f in LISTING[:2]:
        assert (on_dir / f).read_bytes() == (off_dir / f).read_bytes(), f
    rd = json.load(open(on_dir / "read_debug.json"))
    assert list(rd) == ["read_mapping_stats", "dual_passing_stats"] and rd["dual_passing_stats"] is None
    details = json.loads(js_on)["gene_details"]
    want = {(g, m["read_qname"]): m for g in ("HLA-A", "HLA-B") for m in details[g]["mapping_details"] if not m["is_ignored"]}
    have = {(g, q): v for g, reads in rd["read_mapping_stats"].items() for q, v in reads.items()}
    assert set(have) == set(want) and len(want) > 60
    fx = sample.fx
    seq_of = {}
    for recs in sample.recs_by_file:
        for r in recs:
            if r[3] == 0 and r[6]:
                seq_of.setdefault(r[2], r[6])
    for key, v in have.items():
        m = want[key]
        assert (v["best_match_id"], v["best_match_star"]) == (m["best_hla_id"], m["best_star_allele"]), key
        assert list(v["mapping_stats"]) == [m["best_hla_id"]]
        st = v["mapping_stats"][m["best_hla_id"]]
        assert st["cdna_mapping"] is None
        dm = st["dna_mapping"]
        assert list(dm) == ["query_len", "target_len", "match_len", "nm", "query_unmapped", "target_unmapped", "cigar", "md"]
        dna = m["best_mapping_stats"]["dna_stats"]
        assert (dm["nm"], dm["target_len"], dm["target_unmapped"]) == (dna["nm"], dna["seq_len"], dna["unmapped"]), key
        check_mapping(dm, seq_of[key[1]], fx.dna_fwd(fx.ids.index(m["best_hla_id"])))


def test_batch_writes_the_single_calls_file(pkg, sample, tmp_path):
    inputs = [dict(bams=sample.bams, vcf=sample.vcf), dict(bams=[sample.hla_bam], vcf=sample.vcf2), dict(bams=sample.bams), dict(vcf=sample.vcf2, sample_name=sample.sample_name)]
    single = []
    for i, kw in enumerate(inputs):
        run(pkg, sample, tmp_path / f"single{i}", True, **kw)
        single.append({f: (tmp_path / f"single{i}" / f).read_bytes() for f in os.listdir(tmp_path / f"single{i}")})
    assert sorted(single[0]) == LISTING and "read_debug.json" in single[1]
    h = pkg.database.Starphase(sample.db, sample.fasta).set_read_debug(True)
    for max_group in (None, 2, 1):
        folders = [str(tmp_path / f"batch{max_group}_{i}") for i in range(len(inputs))]
        for f in folders:
            os.makedirs(f)
        got = h.call_batch(inputs, max_group=max_group, debug_folders=folders)
        assert not any(isinstance(g, Exception) for g in got)
        for i, f in enumerate(folders):
            assert sorted(os.listdir(f)) == sorted(single[i]), (max_group, i)
            for name, want in single[i].items():
                assert open(os.path.join(f, name), "rb").read() == want, (max_group, i, name)
    # the switch is off by default for a batch as well
    h.set_read_debug(False)
    folders = [str(tmp_path / f"off_{i}") for i in range(len(inputs))]
    for f in folders:
        os.makedirs(f)
    h.call_batch(inputs, debug_folders=folders)
    assert sorted(os.listdir(folders[0])) == LISTING[:2]
    h.close()


def test_cli_flag(pkg, sample, tmp_path):
    D = pkg.database
    run(pkg, sample, tmp_path / "api", True, bams=sample.bams, vcf=sample.vcf)
    cmd = [D.cli_path(), "diplotype", "-d", sample.db, "-r", sample.fasta, "-c", sample.vcf, "-b", sample.bams[0], "--bam", sample.bams[1], "-o", str(tmp_path / "calls.json")]
    p = subprocess.run(cmd + ["--debug-reads", "--output-debug", str(tmp_path / "cli")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / "cli")) == LISTING
    for f in LISTING:
        assert (tmp_path / "cli" / f).read_bytes() == (tmp_path / "api" / f).read_bytes(), f
    p = subprocess.run(cmd + ["--debug-reads"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 64 and len(p.stderr.strip().splitlines()) == 1 and "--debug-reads" in p.stderr
    # diplotype-batch: the flag with a manifest that names a debug folder, and without one
    rows = [[str(tmp_path / "b0.json"), ",".join(sample.bams), sample.vcf, "-", "-", "-", str(tmp_path / "bdbg")]]
    man = tmp_path / "samples.tsv"
    man.write_text("\n".join("\t".join(r) for r in rows) + "\n")
    base = [D.cli_path(), "diplotype-batch", "-d", sample.db, "-r", sample.fasta, "--manifest", str(man)]
    p = subprocess.run(base + ["--debug-reads"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert (tmp_path / "bdbg" / "read_debug.json").read_bytes() == (tmp_path / "api" / "read_debug.json").read_bytes()
    rows[0][6] = "-"
    man.write_text("\n".join("\t".join(r) for r in rows) + "\n")
    p = subprocess.run(base + ["--debug-reads"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 64 and len(p.stderr.strip().splitlines()) == 1 and "--debug-reads" in p.stderr
    for sub in ("diplotype", "diplotype-batch"):
        assert "--debug-reads" in subprocess.run([D.cli_path(), sub, "--help"], capture_output=True, text=True).stdout

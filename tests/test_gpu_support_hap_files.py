"""The haplotype lists in the whole-sample calls (sp_starphase_set_support_haplotypes; `--debug-support-haplotypes`; the `support_haplotypes` keyword of Starphase) on the
files of tests/test_gpu_diplotype_files.py.  The switch has effect only where consensus_support.json / cyp2d6_consensus_support.json are written: on, those two files
are the step API's support calls with `haplotypes=True` rendered through the renderers with a list; off -- or alone -- every file and calls.json are the bytes of a
handle that never heard of it; a batch writes each sample's single-call files."""
import json
import os
import subprocess

import numpy as np
import pytest

import cyp_cases_real as cr
from test_gpu_diplotype_files import Sample, fetch_order
from test_gpu_support_ins_files import CONS_CAP, CYP, HLA, files

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sample(pkg, tmp_path_factory):
    return Sample(tmp_path_factory.mktemp("sample"), pkg)


def run(pkg, sample, folder, ctx=None, touch=None, **kw):
    """one whole-sample call with both support switches on; touch: None = the handle never hears of the haplotype switch, else set_support_haplotypes(touch)"""
    h = pkg.database.Starphase(sample.db, sample.fasta, ctx=ctx, debug_folder=str(folder), consensus_support=True, cyp_consensus_support=True)
    if touch is not None:
        h.set_support_haplotypes(touch)
    res = h.call(**kw)
    out = (res.json(), res.pharmcat_tsv())
    h.close()
    return out


def hla_text(pkg, ctx, sample, hla_debug):
    """consensus_support.json from the step API: gene calls, sp_hla_consensus_support_hap per gene, sp_consensus_support_json_hap"""
    from pb_starphase_amd import synth
    D, ffi = pkg.database, pkg.ffi
    dbf, fasta = D.Database(sample.db), D.Fasta(sample.fasta)
    regions = dbf.hla_genes()
    hdb, _alleles = dbf.hla_db(ctx, [fasta.fetch(r["chrom"], r["start"] - 100, r["end"] + 100) for r in regions])
    met = fetch_order(sample, [(r["chrom"], r["start"], r["end"]) for r in regions], D)
    R = ctx.upload([x[2] for x in sorted(met, key=lambda x: x[1])])
    rec = hdb.realign_reads(R)
    calls, is1 = hdb.diplotype_genes(list(range(len(regions))), R, rec)
    entries, targets, all_haps, all_heads = [], [], [], []
    for g, r in enumerate(regions):
        call, cons1, cons2 = calls[g]
        if call.status == 1:
            continue
        side1, side2, (haps, heads) = hdb.consensus_support(g, R, rec, is1, cons1, cons2, haplotypes=True)
        strand = (lambda s: s) if r["is_forward_strand"] else synth.revcomp
        sides = []
        for k, (cons, sup) in enumerate(((cons1, side1), (cons2, side2))):
            if not cons or (k == 1 and not call.is_dual):
                sides.append(None)
                continue
            typed = hla_debug["read_mapping_stats"][r["name"]]["consensus%d" % (k + 1)]["best_match_star"] or None
            sides.append((typed, strand(cons), sup[0], sup[1]))
        e = len(entries)
        entries.append((r["name"], sides))
        haps, heads = haps.copy(), heads.copy()
        haps["target"] += 2 * e                                             # the single call numbers its consensuses 0 and 1
        heads["first_record"] += sum(len(x) for x in all_haps)
        all_haps.append(haps)
        all_heads.append(heads)
        targets.append((2 * e, 2 * e + 1))
    R.close()
    hdb.close()
    haps = np.concatenate(all_haps) if all_haps else np.zeros(0, ffi.HAP_DTYPE)
    heads = np.concatenate(all_heads) if all_heads else np.zeros(0, ffi.HAP_HEAD_DTYPE)
    return ffi.consensus_support_json(entries, haplotypes=(haps, heads), hap_target=targets), ffi.consensus_support_json(entries), len(haps)


def cyp_text(pkg, ctx, sample):
    """cyp2d6_consensus_support.json from the step API: sp_cyp_diplotype_mappings, sp_cyp_consensus_support_hap, sp_cyp_support_json_hap"""
    D = pkg.database
    dbf, fasta = D.Database(sample.db), D.Fasta(sample.fasta)
    w_chrom, _ws, _we = dbf.cyp_window()
    cdb = dbf.cyp_db(ctx, fasta.fetch(w_chrom, sample.locus.start, sample.locus.start + len(sample.locus.sequence)), sample.locus.start)
    cfg, _gd = cr.load_db()
    keys = ("CYP2D6", "CYP2D7", "REP6", "REP7")
    s5 = cfg["cyp2d6_star5_del"]
    lo = min(min(cfg["cyp_coordinates"][k]["start"] for k in keys), s5["start"] - 500)
    hi = max(max(cfg["cyp_coordinates"][k]["end"] for k in keys), s5["end"] + 3000)
    reads = sorted(fetch_order(sample, [("chr22", lo, hi)], D), key=lambda x: x[1])
    R = ctx.upload([r[2] for r in reads])
    call, cons, mappings = D.cyp_call_with_consensus(cdb, R, CONS_CAP)
    assert call.status == 0 and len(mappings) > 0
    cols, sums, (haps, heads) = D.cyp_consensus_support(ctx, R, call, cons, CONS_CAP, mappings, haplotypes=True)
    text = [D.cyp_consensus_of(cons, CONS_CAP, h) for h in range(call.n_consensus)]
    return D.cyp_support_json(call, text, cols, sums, haplotypes=(haps, heads)), D.cyp_support_json(call, text, cols, sums), len(haps)


def haplotype_entries(text):
    """(path, haplotypes) of every consensus / region of a support file that carries the key"""
    out = []

    def walk(node, path):
        if isinstance(node, dict):
            if "contested" in node:
                if "haplotypes" in node:
                    out.append((path, node["haplotypes"], node))
            else:
                for k, v in node.items():
                    walk(v, path + (k,))
    walk(json.loads(text), ())
    return out


@pytest.fixture(scope="module")
def runs(pkg, gpu_ctx, sample, tmp_path_factory):
    root = tmp_path_factory.mktemp("runs")
    kw = dict(bams=sample.bams, vcf=sample.vcf)
    out = {name: run(pkg, sample, root / name, touch=touch, **kw) for name, touch in (("never", None), ("off", False), ("on", True))}
    return dict(root=root, out=out, files={name: files(root / name) for name in out}, kw=kw)


def test_switch_on_the_files_carry_the_step_apis_haplotypes(pkg, gpu_ctx, sample, runs):
    f_on, f_never = runs["files"]["on"], runs["files"]["never"]
    assert sorted(f_on) == sorted(f_never) and HLA in f_on and CYP in f_on
    assert {k: v for k, v in f_on.items() if k not in (HLA, CYP)} == {k: v for k, v in f_never.items() if k not in (HLA, CYP)}
    assert runs["out"]["on"] == runs["out"]["never"]                                        # calls.json and the TSV: the same bytes
    listed = 0
    for name, (with_list, without, n_haps) in ((HLA, hla_text(pkg, gpu_ctx, sample, json.loads(f_on["hla_debug.json"]))), (CYP, cyp_text(pkg, gpu_ctx, sample))):
        text = f_on[name].decode()
        assert text == json.dumps(json.loads(text), indent=2)                               # the file parses, in the layout of the other debug files
        assert text == with_list, name
        assert f_never[name].decode() == without, name
        assert ("haplotypes" in text) == (n_haps > 0)
        for path, hap, node in haplotype_entries(text):                                     # what the key holds wherever an entry has it
            listed += 1
            assert hap["columns"] == [c["pos"] for c in node["contested"]][:64] and hap["columns_total"] == node["n_contested"]
            assert 1 <= len(hap["patterns"]) <= 16 and sum(p["count"] for p in hap["patterns"]) + hap.get("more", 0) == node["n_aligned"]
            assert all(set(p["calls"]) <= set("=ACGT-?+") for p in hap["patterns"])
    # every consensus or region with a contested column and an aligned member carries the key
    due = sum(text.count('"contested": [\n') for text in (f_on[HLA].decode(), f_on[CYP].decode()))
    assert listed == due


def test_switch_off_is_a_handle_that_never_heard_of_it(pkg, gpu_ctx, sample, runs, tmp_path):
    assert runs["files"]["off"] == runs["files"]["never"] and runs["out"]["off"] == runs["out"]["never"]
    assert HLA in runs["files"]["never"] and CYP in runs["files"]["never"]
    # alone the switch writes nothing: neither file, and every other byte as without it
    h = pkg.database.Starphase(sample.db, sample.fasta, debug_folder=str(tmp_path / "alone"), support_haplotypes=True)
    res = h.call(**runs["kw"])
    assert (res.json(), res.pharmcat_tsv()) == runs["out"]["never"]
    h.close()
    alone = files(tmp_path / "alone")
    assert HLA not in alone and CYP not in alone and alone == {k: v for k, v in runs["files"]["never"].items() if k not in (HLA, CYP)}
    # on a caller's context: off, a warm call launches none of the list's kernels and takes no pool memory; on, it does
    h = pkg.database.Starphase(sample.db, sample.fasta, ctx=gpu_ctx, debug_folder=str(tmp_path / "warm"), consensus_support=True, cyp_consensus_support=True)
    h.set_support_haplotypes(True)
    h.call(**runs["kw"])
    assert files(tmp_path / "warm")[HLA] == runs["files"]["on"][HLA] and files(tmp_path / "warm")[CYP] == runs["files"]["on"][CYP]
    h.set_support_haplotypes(False)
    h.call(**runs["kw"])
    before, launches = gpu_ctx.profile_get("pool:device"), gpu_ctx.profile_get("support_hap")[1]
    assert launches > 0
    h.call(**runs["kw"])
    assert gpu_ctx.profile_get("pool:device") == before and gpu_ctx.profile_get("support_hap")[1] == launches
    assert files(tmp_path / "warm") == runs["files"]["never"]
    h.close()


def test_with_the_insertion_switch_both_lists_are_written(pkg, sample, runs, tmp_path):
    h = pkg.database.Starphase(sample.db, sample.fasta, debug_folder=str(tmp_path / "both"), consensus_support=True, cyp_consensus_support=True, support_insertions=True,
                               support_haplotypes=True)
    h.call(**runs["kw"])
    h.close()
    h = pkg.database.Starphase(sample.db, sample.fasta, debug_folder=str(tmp_path / "ins"), consensus_support=True, cyp_consensus_support=True, support_insertions=True)
    h.call(**runs["kw"])
    h.close()
    both, ins = files(tmp_path / "both"), files(tmp_path / "ins")

    def without(node):
        if isinstance(node, dict):
            return {k: without(v) for k, v in node.items() if k != "haplotypes"}
        return [without(v) for v in node] if isinstance(node, list) else node
    for name in (HLA, CYP):
        assert [h for _p, h, _n in haplotype_entries(both[name].decode())] == [h for _p, h, _n in haplotype_entries(runs["files"]["on"][name].decode())]
        assert json.dumps(without(json.loads(both[name])), indent=2).encode() == ins[name]


def test_batch_files_equal_the_single_calls(pkg, sample, runs, tmp_path):
    inputs = [runs["kw"], dict(bams=[sample.hla_bam], vcf=sample.vcf2), dict(bams=sample.bams)]
    single = [runs["files"]["on"]]
    for i, kw in enumerate(inputs[1:], 1):
        run(pkg, sample, tmp_path / f"single{i}", touch=True, **kw)
        single.append(files(tmp_path / f"single{i}"))
    h = pkg.database.Starphase(sample.db, sample.fasta, consensus_support=True, cyp_consensus_support=True, support_haplotypes=True)
    for max_group in (1, 3):
        folders = [str(tmp_path / f"batch{max_group}_{i}") for i in range(len(inputs))]
        for f in folders:
            os.makedirs(f)
        got = h.call_batch(inputs, max_group=max_group, debug_folders=folders)
        assert not any(isinstance(g, Exception) for g in got)
        for i, f in enumerate(folders):
            assert files(f) == single[i], (max_group, i)
    h.close()


def test_cli_flag(pkg, sample, runs, tmp_path):
    D = pkg.database
    cmd = [D.cli_path(), "diplotype", "-d", sample.db, "-r", sample.fasta, "-c", sample.vcf, "-b", sample.bams[0], "--bam", sample.bams[1], "-o", str(tmp_path / "calls.json"),
           "--debug-consensus-support", "--debug-cyp2d6-support", "--debug-support-haplotypes", "--output-debug", str(tmp_path / "cli")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert files(tmp_path / "cli") == runs["files"]["on"]
    rows = [[str(tmp_path / "b0.json"), ",".join(sample.bams), sample.vcf, "-", "-", "-", str(tmp_path / "bdbg")]]
    man = tmp_path / "samples.tsv"
    man.write_text("\n".join("\t".join(r) for r in rows) + "\n")
    p = subprocess.run([D.cli_path(), "diplotype-batch", "-d", sample.db, "-r", sample.fasta, "--manifest", str(man), "--debug-consensus-support", "--debug-cyp2d6-support",
                        "--debug-support-haplotypes"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert files(tmp_path / "bdbg") == runs["files"]["on"]
    for sub in ("diplotype", "diplotype-batch"):
        assert "--debug-support-haplotypes" in subprocess.run([D.cli_path(), sub, "--help"], capture_output=True, text=True).stdout

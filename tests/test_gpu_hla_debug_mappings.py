"""hla_debug.json's per-allele mappings in the whole-sample calls (sp_starphase_set_hla_debug_mappings; `--debug-hla-mappings`): for each HLA consensus the mapping against
every allowed allele of its gene, as score_read returns it (src/hla/caller.rs:1332-1511, src/hla/debug.rs:64-183) -- on the files of tests/test_gpu_diplotype_files.py.
The switch is off by default; off it changes nothing, on it changes hla_debug.json only.

Neither the calls JSON nor any other output file carries an HLA consensus or its mapping, so the test takes both from the step-by-step path of
tests/test_gpu_diplotype_files.py on the same reads (`steps`): sp_hla_realign_reads + sp_hla_diplotype_genes give each gene's consensuses, sp_hla_map_type_consensus
gives each consensus' gene-strand targets and every pair's spans.  Against them every entry of the file is checked exactly: cigar + md applied to the allele from its
a_start reproduce consensus[b_start:b_end], the whole entry is the API's mapping through sp_affine_cigar_strings_eqx, and the typed allele's (len, nm, unmapped) are
sp_hla_best.mm2_stats of sp_hla_type_consensus on that consensus; the typed allele is a haplotype of the calls JSON's diplotype."""
import json
import os
import re
import subprocess

import pytest

from test_gpu_diplotype_files import Sample, fetch_order

pytestmark = pytest.mark.gpu
FIELDS = ["query_len", "target_len", "match_len", "nm", "query_unmapped", "target_unmapped", "cigar", "md"]


@pytest.fixture(scope="module")
def sample(pkg, tmp_path_factory):
    return Sample(tmp_path_factory.mktemp("sample"), pkg)


class Steps:
    """the step-by-step path on the sample's reads: per gene the call and its consensuses, and (per settings) the API's map of each consensus"""

    def __init__(self, pkg, ctx, sample):
        D = pkg.database
        dbf, fasta = D.Database(sample.db), D.Fasta(sample.fasta)
        self.D, self.regions = D, dbf.hla_genes()
        gene_ref = [fasta.fetch(r["chrom"], r["start"] - 100, r["end"] + 100) for r in self.regions]
        self.hdb, self.alleles = dbf.hla_db(ctx, gene_ref)
        met = fetch_order(sample, [(r["chrom"], r["start"], r["end"]) for r in self.regions], D)
        R = ctx.upload([x[2] for x in sorted(met, key=lambda x: x[1])])
        rec = self.hdb.realign_reads(R)
        self.calls, _ = self.hdb.diplotype_genes(list(range(len(self.regions))), R, rec)
        self._maps = {}

    def map(self, g, k, require_dna, no_cdna):
        """(HlaMap, mm2_stats of sp_hla_type_consensus) of consensus k + 1 of gene g"""
        key = (g, k, require_dna, no_cdna)
        if key not in self._maps:
            cons = self.calls[g][1 + k]
            m = self.hdb.map_type_consensus(g, cons, require_dna=require_dna, disable_cdna=no_cdna)
            best = self.hdb.type_consensus(g, cons, require_dna=require_dna, disable_cdna=no_cdna, stats=False)[0]
            self._maps[key] = (m, int(best), list(self.hdb.last_mm2_stats))
        return self._maps[key]


@pytest.fixture(scope="module")
def hdb(pkg, gpu_ctx, sample):
    return Steps(pkg, gpu_ctx, sample)


def run(pkg, sample, folder, on, touch=True, settings=None, read_debug=False, **kw):
    h = pkg.database.Starphase(sample.db, sample.fasta, debug_folder=str(folder), **(settings or {}))
    if read_debug:
        h.set_read_debug(True)
    if touch:
        h.set_hla_debug_mappings(on)
    res = h.call(**kw)
    out = (res.json(), res.pharmcat_tsv(), h.warnings())
    h.close()
    return out


def files(folder):
    return {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))}


def rebuild(dm, allele, qs):
    """the consensus bases a (cigar, md) pair spells when the mapping starts at allele base qs: '=' columns are the allele's bases, 'X' and 'D' columns are MD's"""
    md = re.findall(r"(\d+)|\^([ACGTN]+)|([ACGTN])", dm["md"])
    md_x = [m[2] for m in md if m[2]]; md_d = [m[1] for m in md if m[1]]
    out, q, xi, di = [], qs, 0, 0
    d_bases = "".join(md_d)
    for n, op in [(int(n), op) for n, op in re.findall(r"(\d+)([=XID])", dm["cigar"])]:
        if op == "=":
            out.append(allele[q:q + n]); q += n
        elif op == "X":
            out.append("".join(md_x[xi:xi + n])); xi += n; q += n
        elif op == "I":
            q += n
        else:
            out.append(d_bases[di:di + n]); di += n
    assert xi == len(md_x) and di == len(d_bases) and q - qs == dm["query_len"] - dm["query_unmapped"]
    return "".join(out)


def check_entry(dm, allele):
    """nm = X + I + D bases, match_len = '=' bases, the unmapped counts = lengths minus spans, MD's matches are the CIGAR's"""
    assert list(dm) == FIELDS
    runs = [(int(n), op) for n, op in re.findall(r"(\d+)([=XID])", dm["cigar"])]
    assert "".join(f"{n}{op}" for n, op in runs) == dm["cigar"] and runs and all(a[1] != b[1] for a, b in zip(runs, runs[1:]))
    by = {op: sum(n for n, o in runs if o == op) for op in "=XID"}
    assert dm["nm"] == by["X"] + by["I"] + by["D"]
    assert dm["match_len"] == by["="]
    assert dm["query_len"] == len(allele)
    assert dm["query_unmapped"] == dm["query_len"] - (by["="] + by["X"] + by["I"])
    assert dm["target_unmapped"] == dm["target_len"] - (by["="] + by["X"] + by["D"])
    assert sum(int(n) for n in re.findall(r"\d+", dm["md"])) == by["="]


def check_file(steps, sample, dbg, calls_json, warnings, require_dna=False, no_cdna=False):
    fx, D = sample.fx, steps.D
    rms = dbg["read_mapping_stats"]
    diplo = json.loads(calls_json)["gene_details"]
    assert sorted(rms) == ["HLA-A", "HLA-B"]
    fx_of = {hid: i for i, hid in enumerate(fx.ids)}
    n_entries = 0
    for gene, per in rms.items():
        g = [r["name"] for r in steps.regions].index(gene)
        call = steps.calls[g][0]
        assert per and list(per) == (["consensus1", "consensus2"] if call.is_dual else ["consensus1"])
        skipped = [ln for ln in warnings.splitlines() if ln.startswith(f"hla_debug.json: {gene} ")]
        haps = {h for d in diplo[gene]["diplotypes"] for h in (d["hap1"], d["hap2"])}
        for k, (who, rec) in enumerate(per.items()):
            ms = rec["mapping_stats"]
            m, best, mm2 = steps.map(g, k, require_dna, no_cdna)
            # one entry per allowed allele: per star allele; the alleles that repeat one are skipped with a warning each
            first_of = {}
            for x, a in enumerate(m.alleles):
                first_of.setdefault(steps.alleles[int(a)][2], x)
            gi = fx.genes.index(gene)
            assert sorted(fx_of[steps.alleles[int(a)][0]] for a in m.alleles) == [a for a in range(len(fx.ids)) if fx.gene_of[a] == gi and (fx.dna[a] or not require_dna)]
            assert set(ms) == set(first_of), (gene, who, len(ms), len(first_of))
            assert len(ms) + sum(1 for ln in skipped if f" {who}: " in ln) == len(m.alleles)
            # the typed allele: the step path's, a haplotype of the calls JSON's diplotype, with the (len, nm, unmapped) sp_hla_type_consensus reports for the winner
            typed = rec["best_match_star"].split("*", 1)[1]
            assert rec["best_match_id"] == steps.alleles[best][0] and steps.alleles[best][2] == typed and best == (call.typed2 if k else call.typed1)
            assert "*" + typed in haps, (gene, who, typed, haps)
            want = []
            for key in ("cdna_mapping", "dna_mapping"):
                dm = ms[typed][key]
                want += [-1, -1, -1] if dm is None else [dm["query_len"], dm["nm"], dm["query_unmapped"]]
            assert want == mm2, (gene, who, want, mm2)
            # every entry: the API's mapping, and cigar + md applied to the allele from a_start give the consensus over [b_start, b_end)
            for star, st in ms.items():
                x = first_of[star]
                fa = fx_of[steps.alleles[int(m.alleles[x])][0]]
                assert list(st) == ["cdna_mapping", "dna_mapping"]
                for lv, key, seqs, cons in ((0, "cdna_mapping", fx.cdna, m.cons_cdna), (1, "dna_mapping", fx.dna, m.cons_dna)):
                    dm, al = st[key], m.aln[lv, x]
                    if al["score"] <= 0 or (lv == 0 and no_cdna):
                        assert dm is None, (gene, who, star, key)
                        continue
                    allele = seqs[fa]
                    check_entry(dm, allele)
                    cg, md, ml = D.affine_cigar_strings_eqx(al, m.cigar[lv][x], cons)
                    assert dm == dict(query_len=len(allele), target_len=len(cons), match_len=ml, nm=int(al["nm"]), query_unmapped=len(allele) - int(al["a_end"] - al["a_start"]),
                                      target_unmapped=len(cons) - int(al["b_end"] - al["b_start"]), cigar=cg, md=md), (gene, who, star, key)
                    assert rebuild(dm, allele, int(al["a_start"])) == cons[int(al["b_start"]):int(al["b_end"])], (gene, who, star, key)
                    n_entries += 1
    return n_entries


def test_switch_off_and_on(pkg, sample, hdb, tmp_path):
    kw = dict(bams=sample.bams, vcf=sample.vcf)
    never = run(pkg, sample, tmp_path / "never", False, touch=False, read_debug=True, **kw)
    off = run(pkg, sample, tmp_path / "off", False, read_debug=True, **kw)
    on = run(pkg, sample, tmp_path / "on", True, read_debug=True, **kw)
    f_never, f_off, f_on = files(tmp_path / "never"), files(tmp_path / "off"), files(tmp_path / "on")
    assert sorted(f_never) == ["cyp2d6_alleles.json", "hla_debug.json", "read_debug.json"]
    # off: everything is the same bytes as a run that never touched the switch
    assert off[:2] == never[:2] and f_off == f_never
    assert all(r["mapping_stats"] == {} for per in json.loads(f_off["hla_debug.json"])["read_mapping_stats"].values() for r in per.values())
    # on: everything but hla_debug.json
    assert on[:2] == never[:2]
    assert {k: v for k, v in f_on.items() if k != "hla_debug.json"} == {k: v for k, v in f_never.items() if k != "hla_debug.json"}
    dbg_on, dbg_off = json.loads(f_on["hla_debug.json"]), json.loads(f_off["hla_debug.json"])
    assert dbg_on["dual_passing_stats"] == dbg_off["dual_passing_stats"]
    for gene, per in dbg_on["read_mapping_stats"].items():
        for who, rec in per.items():
            assert {k: v for k, v in rec.items() if k != "mapping_stats"} == {k: v for k, v in dbg_off["read_mapping_stats"][gene][who].items() if k != "mapping_stats"}
    n = check_file(hdb, sample, dbg_on, on[0], on[2])
    print("\nhla_debug.json: mappings checked", n, "; bytes", len(f_on["hla_debug.json"]), "; warnings", len(on[2].splitlines()))
    assert n > 20000


def test_single_call_equals_batch_for_any_group_size(pkg, sample, tmp_path):
    inputs = [dict(bams=sample.bams, vcf=sample.vcf), dict(bams=[sample.hla_bam], vcf=sample.vcf2), dict(bams=sample.bams), dict(vcf=sample.vcf2, sample_name=sample.sample_name)]
    single = []
    for i, kw in enumerate(inputs):
        run(pkg, sample, tmp_path / f"single{i}", True, **kw)
        single.append(files(tmp_path / f"single{i}"))
    assert b'"cigar"' in single[0]["hla_debug.json"] and b'"cigar"' in single[1]["hla_debug.json"]
    h = pkg.database.Starphase(sample.db, sample.fasta).set_hla_debug_mappings(True)
    for max_group in (None, 2, 1):
        folders = [str(tmp_path / f"batch{max_group}_{i}") for i in range(len(inputs))]
        for f in folders:
            os.makedirs(f)
        got = h.call_batch(inputs, max_group=max_group, debug_folders=folders)
        assert not any(isinstance(g, Exception) for g in got)
        for i, f in enumerate(folders):
            assert files(f) == single[i], (max_group, i)
    h.close()


def test_cli_flag_and_disabled_cdna(pkg, sample, hdb, tmp_path):
    D = pkg.database
    run(pkg, sample, tmp_path / "api", True, bams=sample.bams, vcf=sample.vcf)
    cmd = [D.cli_path(), "diplotype", "-d", sample.db, "-r", sample.fasta, "-c", sample.vcf, "-b", sample.bams[0], "--bam", sample.bams[1], "-o", str(tmp_path / "calls.json")]
    p = subprocess.run(cmd + ["--debug-hla-mappings", "--output-debug", str(tmp_path / "cli")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert files(tmp_path / "cli") == files(tmp_path / "api")
    p = subprocess.run(cmd + ["--debug-hla-mappings"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 64 and len(p.stderr.strip().splitlines()) == 1 and "--debug-hla-mappings" in p.stderr
    rows = [[str(tmp_path / "b0.json"), ",".join(sample.bams), sample.vcf, "-", "-", "-", str(tmp_path / "bdbg")]]
    man = tmp_path / "samples.tsv"
    man.write_text("\n".join("\t".join(r) for r in rows) + "\n")
    base = [D.cli_path(), "diplotype-batch", "-d", sample.db, "-r", sample.fasta, "--manifest", str(man)]
    p = subprocess.run(base + ["--debug-hla-mappings"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert (tmp_path / "bdbg" / "hla_debug.json").read_bytes() == (tmp_path / "api" / "hla_debug.json").read_bytes()
    rows[0][6] = "-"
    man.write_text("\n".join("\t".join(r) for r in rows) + "\n")
    p = subprocess.run(base + ["--debug-hla-mappings"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 64 and len(p.stderr.strip().splitlines()) == 1 and "--debug-hla-mappings" in p.stderr
    for sub in ("diplotype", "diplotype-batch"):
        assert "--debug-hla-mappings" in subprocess.run([D.cli_path(), sub, "--help"], capture_output=True, text=True).stdout
    # --disable-cdna-scoring --hla-require-dna: no cDNA mapping, the alleles with DNA only
    js, _tsv, warn = run(pkg, sample, tmp_path / "nocdna", True, settings=dict(disable_cdna_scoring=1, hla_require_dna=1), bams=sample.bams, vcf=sample.vcf)
    dbg = json.loads(files(tmp_path / "nocdna")["hla_debug.json"])
    assert all(st["cdna_mapping"] is None for per in dbg["read_mapping_stats"].values() for rec in per.values() for st in rec["mapping_stats"].values())
    assert check_file(hdb, sample, dbg, js, warn, require_dna=True, no_cdna=True) > 5000
    p = subprocess.run(cmd + ["--debug-hla-mappings", "--disable-cdna-scoring", "--hla-require-dna", "--output-debug", str(tmp_path / "cli_nocdna")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert files(tmp_path / "cli_nocdna")["hla_debug.json"] == files(tmp_path / "nocdna")["hla_debug.json"]

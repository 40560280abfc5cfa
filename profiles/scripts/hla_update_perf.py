"""sp_hla_config_extend over every DNA allele of the bundled database (tests/golden/hla_db_v0.14.1.json.gz) against the two chr6 islands, beside HlaConfig::new on
the minimap2 restatement (oracle/mm2.c, one thread): both times, the alleles whose records differ, the final coordinates.
usage: hla_update_perf.py [--oracle-only FILE | --oracle FILE] [--divergence FILE] [--batch N]
  --oracle-only FILE   run the CPU side alone and keep its records in FILE (no device needed)
  --oracle FILE        take the CPU side's records and time from FILE instead of running it"""
import gzip
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hla_update_cases as hc          # noqa: E402
import test_oracle_mm2 as tm           # noqa: E402

FIELDS = ("rev", "nm", "q_start", "q_end", "t_start", "t_end")


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    seqs = json.load(gzip.open(os.path.join(hc.GOLDEN, "hla_db_v0.14.1.json.gz")))
    seqs = seqs.get("hla_sequences", seqs)
    alleles = [(a["gene_name"], "db", a["gene_name"][4:] + "*" + ":".join(a["star_allele"]) + "|" + k, a["dna_sequence"], a["cdna_sequence"]) for k, a in sorted(seqs.items())
               if a["gene_name"] in hc.REFSEQ]
    ids = {a[2]: a[2].split("|")[1] for a in alleles}
    n_dna = sum(1 for a in alleles if a[3])
    print(f"{len(alleles)} alleles of HLA-A / HLA-B, {n_dna} with DNA")
    cache = arg("--oracle") or arg("--oracle-only")
    if arg("--oracle") and os.path.exists(cache):
        o = json.load(open(cache))
        want_recs, want_genes, cpu_s = o["recs"], {g: tuple(v) for g, v in o["genes"].items()}, o["seconds"]
    else:
        mm = tm.mm2_ffi.Mm2()
        t0 = time.perf_counter()
        want_recs, want_genes = hc.oracle_extend(mm, alleles, ids)
        cpu_s = time.perf_counter() - t0
        if cache:
            json.dump(dict(recs=want_recs, genes=want_genes, seconds=cpu_s), open(cache, "w"))
    print(f"oracle (minimap2 restatement, one thread): {cpu_s:.2f} s, {cpu_s / n_dna * 1e3:.2f} ms per allele")
    print("oracle coordinates:", {g: v[:3] for g, v in want_genes.items()}, "worst:", {g: v[3:] for g, v in want_genes.items()})
    if arg("--oracle-only"):
        return
    import __graft_entry__ as ge
    pkg = ge.load_package()
    D = pkg.database
    with tempfile.TemporaryDirectory() as tmp:
        from pathlib import Path
        tmp = Path(tmp)
        gen = hc.write_fasta(tmp / "gen.fa", [(ids[d], d.split("|")[0], s) for _g, _k, d, s, _c in alleles if s])
        nuc = hc.write_fasta(tmp / "nuc.fa", [(ids[d], d.split("|")[0], c) for _g, _k, d, _s, c in alleles])
        (tmp / "db.json").write_text(json.dumps(hc.refseq_database()))
        chr6 = hc.write_chr6(tmp / "chr6.fa")
        t0 = time.perf_counter()
        A = D.HlaAlleles.load(gen, nuc)
        load_s = time.perf_counter() - t0
        ctx = pkg.Context(0)
        fasta, db = D.Fasta(chr6), D.Database(tmp / "db.json")
        batch = int(arg("--batch", "0"))
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            R = ctx.hla_config_extend(fasta, A, db, batch_alleles=batch)
            times.append(time.perf_counter() - t0)
        maps = R.mappings()
        print(f"FASTA intake: {load_s:.2f} s;  sp_hla_config_extend (batch {batch or 1024}): " + ", ".join(f"{t:.3f}" for t in times) + f" s  -> {n_dna / min(times):.0f} alleles / s, "
              f"{cpu_s / min(times):.0f}x the one-thread oracle")
        for name in ("hlacfg_anchor", "hlacfg_affine", "hlacfg_pick_extend"):
            ms, launches, cells = ctx.profile_get(name) if hasattr(ctx, "profile_get") else (0, 0, 0)
            print(f"  {name}: {ms:.2f} ms in {launches} launches")
        got = {}
        for i in range(len(A)):
            a = A.allele(i)
            got[a["gene_name"][4:] + "*" + ":".join(a["star_allele"]) + "|" + a["hla_id"]] = maps[i]
        diff = [d for d in got if got[d] != want_recs.get(d)]
        print(f"alleles whose record differs from the oracle's: {len(diff)} of {n_dna} with DNA; reported as none for the band: {len(R.overflow)}")
        print("device coordinates:", {g["name"]: (g["start"], g["end"], g["moved"]) for g in R.genes()},
              "worst:", {g["name"]: (A.allele(g["worst_allele"])["hla_id"] if g["worst_allele"] is not None else None, g["worst"]) for g in R.genes()})
        out = arg("--divergence")
        if out:
            with open(out, "w") as f:
                f.write(f"# sp_hla_config_extend vs HlaConfig::new on the minimap2 restatement: {len(diff)} of {n_dna} DNA alleles of HLA-A / HLA-B (database v0.14.1) differ\n")
                f.write("# allele|id\tdevice record\toracle record\n")
                for d in diff:
                    f.write(f"{d}\t{json.dumps(got[d])}\t{json.dumps(want_recs.get(d))}\n")
        if R.warnings:
            print(R.warnings, end="")


if __name__ == "__main__":
    main()

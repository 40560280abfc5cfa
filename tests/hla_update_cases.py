"""Shared inputs of the update-hla tests (tests/test_hla_fasta.py, tests/test_gpu_hla_update.py): the chr6 islands as a reference FASTA, a database whose hla_config
holds the RefSeq records of HLA-A / HLA-B (the coordinates HlaConfig::new starts from in the reference's own test, src/hla/alleles.rs:512-547), the designed
allele set, and HlaConfig::new over a whole allele table on the minimap2 restatement (the oracle side: test_oracle_mm2.hlaconfig_extend's rule, any number of
alleles per gene)."""
import json
import os

import numpy as np

import test_oracle_mm2 as tm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAUX_GEN = os.path.join(GOLDEN, "HLA-faux", "hla_gen.fa")
FAUX_NUC = os.path.join(GOLDEN, "HLA-faux", "hla_nuc.fa")
BUFFER = 2000
# gene -> (0-based half-open RefSeq record, HlaConfig::default()'s coordinates), from test_oracle_mm2.HLACONFIG_CASES
REFSEQ = {"HLA-" + name[0]: ((s - 1, e), want) for name, s, e, want in tm.HLACONFIG_CASES}
BASE = {"HLA-A": "A*01:01:01:01", "HLA-B": "B*07:02:01:01"}


def read_fasta(path):
    """{id: (description word, sequence)} of a FASTA file, by the simplest reading of the format"""
    out, key = {}, None
    for line in open(path):
        line = line.strip()
        if line.startswith(">"):
            key = line[1:].split()[0]
            out[key] = [line[1:].split()[1], []]
        elif line:
            out[key][1].append(line)
    return {k: (d, "".join(s)) for k, (d, s) in out.items()}


def write_fasta(path, records):
    """records: [(id, description, sequence)], 60 bases per line as IMGT writes them"""
    with open(path, "w") as f:
        for rid, desc, seq in records:
            f.write(f">{rid} {desc} {len(seq)} bp\n")
            f.writelines(seq[i:i + 60] + "\n" for i in range(0, len(seq), 60))
    return str(path)


def write_chr6(path):
    """chr6 up to the end of the second island as an indexed FASTA: N everywhere but the two islands (one line; the index makes a fetch read its bases only)"""
    isl = tm._islands()
    parts, at = [], 0
    for (s, e), seq in sorted(isl.items()):
        parts += ["N" * (s - at), seq]
        at = e
    seq = "".join(parts)
    with open(path, "w") as f:
        f.write(">chr6\n" + seq + "\n")
    open(str(path) + ".fai", "w").write(f"chr6\t{len(seq)}\t6\t{len(seq)}\t{len(seq) + 1}\n")
    return str(path)


def gene_definition(name, chrom, start, end, forward, exons, transcript=None):
    return {"gene_name": name, "coordinates": {"chrom": chrom, "start": start, "end": end}, "is_forward_strand": forward, "transcript_id": transcript,
            "exons": [{"chrom": chrom, "start": s, "end": e} for s, e in exons], "is_absent_capable": False}


def refseq_database(extra_genes=(), variant_db=None):
    """the faux database (as a dict) with an hla_config in the v1.0 form whose genes carry the RefSeq coordinates; exons are the default's (RefSeq's own)"""
    db = json.load(open(os.path.join(GOLDEN, "hla_faux_database.json")))
    exons = {"HLA-A": [(29942531, 29942626), (29942756, 29943026), (29943267, 29943543), (29944121, 29944397), (29944499, 29944616), (29945058, 29945091),
                       (29945233, 29945281), (29945450, 29945870)],
             "HLA-B": [(31353874, 31354296), (31354478, 31354526), (31354632, 31354665), (31355106, 31355223), (31355316, 31355592), (31356166, 31356442),
                       (31356687, 31356957), (31357085, 31357179)]}
    genes = {g: gene_definition(g, "chr6", s, e, g == "HLA-A", exons[g], {"HLA-A": "NM_002116.8", "HLA-B": "NM_005514.8"}[g]) for g, ((s, e), _w) in REFSEQ.items()}
    for g in extra_genes:
        genes[g["gene_name"]] = g
    db["hla_config"] = {"gene_collection": {"version": "NCBI RefSeq test", "gene_dict": genes}}
    if variant_db:
        db["gene_entries"] = json.load(open(os.path.join(GOLDEN, "variant_dbs", variant_db + ".json")))["gene_entries"]
    return db


def windows():
    """gene -> (window start on chr6, window bases): the RefSeq record +- 2,000 bases"""
    out = {}
    for g, ((s, e), _w) in REFSEQ.items():
        (i0, i1), seq = next((k, v) for k, v in tm._islands().items() if k[0] <= s - BUFFER and e + BUFFER <= k[1])
        out[g] = (s - BUFFER, seq[s - BUFFER - i0:e + BUFFER - i0])
    return out


def designed_set(mm):
    """[(gene, kind, star description, dna or None, cdna)]: eight derivatives of each of the two real alleles (the kinds below), in a fixed order"""
    gen, nuc = read_fasta(FAUX_GEN), read_fasta(FAUX_NUC)
    by_desc = {d: (s, nuc[k][1]) for k, (d, s) in gen.items()}
    win = windows()
    out = []
    for gi, gene in enumerate(("HLA-A", "HLA-B")):
        letter = gene[-1]
        dna, cdna = by_desc[BASE[gene]]
        rng = np.random.default_rng(4100 + gi)
        w0, target = win[gene]
        m = mm.map_pair(target, dna)[0]                                        # where the allele lies on the window: the flank bases come from there
        left, right = target[m["t_start"] - 60:m["t_start"]], target[m["t_end"]:m["t_end"] + 60]
        assert m["q_start"] == 0 and m["q_end"] == len(dna)
        flanked = left + dna + right if not m["rev"] else tm.revcomp(left + tm.revcomp(dna) + right)
        subs = list(dna)
        for p in rng.choice(np.arange(100, len(dna) - 100), size=round(0.005 * len(dna)), replace=False):
            subs[p] = "ACGT"[("ACGT".index(subs[p]) + 1 + int(rng.integers(0, 3))) % 4]
        mid = len(dna) // 2
        kinds = [("unchanged", dna), ("cut5", dna[40:]), ("cut3", dna[:-40]), ("flank60", flanked), ("subs", "".join(subs)), ("del12", dna[:mid] + dna[mid + 12:]),
                 ("random", tm.rnd(rng, 3500)), ("cdna_only", None)]
        for k, (kind, seq) in enumerate(kinds):
            out.append((gene, kind, f"{letter}*{90 + k}:01:01:01", seq, cdna))
    return out


def write_set(tmp, alleles, order=None, tag="set"):
    """the set as two FASTA files with ids HLA:HLA9xxxx given in `order` (a permutation of the set: position p of the id sequence goes to allele order[p]);
    -> (gen path, nuc path, {star description: hla id})"""
    order = list(range(len(alleles))) if order is None else list(order)
    ids = {}
    for p, a in enumerate(order):
        ids[alleles[a][2]] = f"HLA:HLA9{p:04d}"
    gen = [(ids[d], d, s) for _g, _k, d, s, _c in alleles if s is not None]
    nuc = [(ids[d], d, c) for _g, _k, d, _s, c in alleles]
    return write_fasta(tmp / f"{tag}_gen.fa", gen), write_fasta(tmp / f"{tag}_nuc.fa", nuc), ids


def oracle_extend(mm, alleles, ids, require_single=False):
    """HlaConfig::new (src/hla/alleles.rs:109-207) on the minimap2 restatement: alleles visited in id order; per allele the mapping with the strictly smallest
    (nm + unmapped) / len below 1.0, first wins; the gene's coordinates extended over it; the worst accepted score replaces on strictly greater.
    -> ({star description: record or None}, {gene: (start, end, moved, worst description or None, worst (len, nm, unmapped) or None)})"""
    recs, genes = {}, {}
    for gene, (w0, target) in windows().items():
        (start, end), _want = REFSEQ[gene]
        s, e = start, end
        worst, worst_score, worst_stats = None, 0.1 / len(target), None           # MappingStats::new(ref_len, 0, 0)
        for g, _kind, desc, dna, _c in sorted((a for a in alleles if a[0] == gene), key=lambda a: ids[a[2]]):
            if dna is None:
                recs[desc] = None
                continue
            best, best_score, best_stats = None, 1.0, None
            maps = mm.map_pair(target, dna)
            for m in maps:
                unmapped = len(dna) - (m["q_end"] - m["q_start"])
                score = max(m["nm"] + unmapped, 0.1) / len(dna)
                if score < best_score:
                    best, best_score, best_stats = m, score, (len(dna), m["nm"], unmapped)
            if require_single and best is not None:
                assert sum(1 for m in maps if m["rev"] == best["rev"]) == 1, (desc, maps)
            recs[desc] = None if best is None else {k: int(best[k]) for k in ("rev", "nm", "q_start", "q_end", "t_start", "t_end")}
            if best is not None:
                s, e = min(s, w0 + best["t_start"]), max(e, w0 + best["t_end"])
                if best_score > worst_score:
                    worst, worst_score, worst_stats = desc, best_score, best_stats
        genes[gene] = (s, e, (s, e) != (start, end), worst, worst_stats)
    return recs, genes

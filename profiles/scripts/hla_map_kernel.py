"""kernel comparison: the K2 map path against sp_affine_align_batch over the same pairs (four configs[1] consensuses, all pairs), median of five, alternating"""
import gzip, json, os, sys, time, zlib
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge
pkg = ge.load_package()
from pb_starphase_amd import synth
gold = json.load(gzip.open(os.path.join(ROOT, "tests", "golden", "concordance.json.gz"), "rt"))
ctx = pkg.Context(0)
fx = synth.HlaFixture(); db = fx.make_db(pkg, ctx)
items = []
for row in gold["k2"]["consensuses"]:
    gi = fx.genes.index(row["gene"])
    cons = [c for c in gold["hla"]["consensus"][row["gene"]] if zlib.crc32(c.encode()) & 0xFFFFFFFF == row["consensus_crc"]][0]
    m = db.map_type_consensus(gi, cons)
    items.append((gi, m.cons_dna, m.cons_cdna, m))
# the baseline's inputs: per level one allele set, one consensus set, the pairs of the map
base = []
for lv, seqs in ((0, fx.cdna), (1, fx.dna)):
    a_list, pairs, b_list = [], [], []
    for ci, (gi, _d, _c, m) in enumerate(items):
        b_list.append(m.cons_cdna if lv == 0 else m.cons_dna)
        for k in range(len(m.alleles)):
            if m.aln[lv, k]["score"] > 0:
                pairs.append((len(a_list), ci, int(m.diag[lv, k]))); a_list.append(seqs[int(m.alleles[k])])
    base.append((ctx.upload(a_list), ctx.upload(b_list), pairs))
n_pairs = sum(len(b[2]) for b in base)
def run_map():
    ctx.profile_reset(); t = time.perf_counter()
    db.map_consensus_batch([(g, d, c) for g, d, c, _m in items])
    wall = (time.perf_counter() - t) * 1e3
    return ctx.profile_get("k2_map_cdna")[0] + ctx.profile_get("k2_map_dna")[0], wall
def run_base():
    ctx.profile_reset(); t = time.perf_counter()
    for A, B, pairs in base:
        ctx.affine_align(A, B, pairs, a=5, band=64, cigar_stride=768)
    wall = (time.perf_counter() - t) * 1e3
    return ctx.profile_get("affine_align")[0], wall
# how often the op buffer's starting guess (24 words a pair and level) was too small: launches of the two map kernels in the first (cold) and the second call
ctx.profile_reset(); db.map_consensus_batch([(g, d, c) for g, d, c, _m in items])
print("map launches of a first batched call (2 = no second run):", ctx.profile_get("k2_map_cdna")[1] + ctx.profile_get("k2_map_dna")[1],
      "; ops per mapped pair: %.1f" % (sum(len(c) for _g, _d, _c, m in items for lv in (0, 1) for c in m.cigar[lv]) / max(1, n_pairs)))
run_map(); run_base()
ctx.profile_reset(); db.map_consensus_batch([(g, d, c) for g, d, c, _m in items])
print("map launches of a warm call:", ctx.profile_get("k2_map_cdna")[1] + ctx.profile_get("k2_map_dna")[1])
mm, bb = [], []
for _ in range(5):
    mm.append(run_map()); bb.append(run_base())
def stat(v): v = sorted(v); return "median %.3f min %.3f max %.3f" % (v[len(v) // 2], v[0], v[-1])
# bytes of scratch: baseline = rows x 64 direction bytes + (2 rows + 2) op words per pair; the map = its pooled checkpoint and ring buffers
dir_bytes = 0
for ci, (gi, d, c, m) in enumerate(items):
    for lv in (0, 1):
        tlen = len(m.cons_cdna if lv == 0 else m.cons_dna)
        n = int((m.aln[lv]["score"] > 0).sum())
        dir_bytes += n * (tlen * 64 + (2 * tlen + 2) * 4)
print("pairs", n_pairs)
print("map kernels (k2_map_cdna + k2_map_dna), GPU ms: ", stat([x[0] for x in mm]), " all:", ["%.3f" % x[0] for x in mm])
print("baseline affine_tb_kernel (affine_align), GPU ms:", stat([x[0] for x in bb]), " all:", ["%.3f" % x[0] for x in bb])
print("map call wall ms (whole K2 + map + copies):", stat([x[1] for x in mm]))
print("baseline call wall ms (align_batch only, incl. its hipMalloc/hipFree):", stat([x[1] for x in bb]))
print("baseline direction + op scratch over these pairs, bytes (upper estimate, rows = consensus length):", dir_bytes, "in chunks of up to 536870912")
print("pooled device memory of the context, bytes:", ctx.profile_get("pool:device")[2])
ctx.close()

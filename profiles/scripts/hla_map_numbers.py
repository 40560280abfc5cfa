import gzip, json, os, sys, zlib
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge
pkg = ge.load_package()
from pb_starphase_amd import synth
gold = json.load(gzip.open(os.path.join(ROOT, "tests", "golden", "concordance.json.gz"), "rt"))
ctx = pkg.Context(0)
fx = synth.HlaFixture(); db = fx.make_db(pkg, ctx)
same = either_n = 0
rows_out = []
for row in gold["k2"]["consensuses"]:
    gi = fx.genes.index(row["gene"])
    cons = [c for c in gold["hla"]["consensus"][row["gene"]] if zlib.crc32(c.encode()) & 0xFFFFFFFF == row["consensus_crc"]][0]
    m = db.map_type_consensus(gi, cons)
    port = np.array(row["nm_unmapped"], np.int64); mm2 = m.stats_mm2.astype(np.int64)
    for lv, (cn, cu) in enumerate(((1, 2), (4, 5))):
        p_nm, p_un, l_nm, l_un = port[:, 2 * lv], port[:, 2 * lv + 1], mm2[:, cn], mm2[:, cu]
        either = (p_nm >= 0) | (l_nm >= 0); ok = (p_nm >= 0) & (l_nm >= 0) & (p_nm == l_nm) & (p_un == l_un)
        either_n += int(either.sum()); same += int(ok.sum())
        for k in np.nonzero(either & ~ok)[0]:
            # the divergence classes of DESIGN.md section 3.4
            if l_nm[k] < 0:
                cls = "3.4 edit cap: the port maps the pair; K2's unit-cost cell (255 edits at most) found nothing, so the map has no diagonal to band around"
            elif p_nm[k] < 0:
                cls = "3.4 best_n / seeding: the library maps the pair, the port's chain found nothing"
            elif l_nm[k] > p_nm[k] and l_un[k] >= p_un[k]:
                cls = "3.4 band: the 64 diagonals around the unit-cost cell's midpoint diagonal hold a WORSE path than the port's chain-based alignment (more edits, no more of the allele)"
            elif p_un[k] != l_un[k]:
                cls = "3.4 band / end clipping: another extent than the port's, with FEWER edits (the library's path stops where the port's goes on at up to twice the edits, or ends one base apart)"
            else:
                cls = "3.4 affine against unit-cost optimum: same extent, fewer edits than the port"
            rows_out.append((cls, row["gene"], row["consensus_crc"], fx.ids[int(m.alleles[k])], "cDNA" if lv == 0 else "DNA", (int(l_nm[k]), int(l_un[k])), (int(p_nm[k]), int(p_un[k]))))
print("K2 (allele, level) pairs, mapped by either: %d ; stats_mm2 == the port's (nm, unmapped): %d = %.6f" % (either_n, same, same / either_n))
print("differing pairs: %d" % len(rows_out))
for cls in sorted(set(r[0] for r in rows_out)):
    sel = [r for r in rows_out if r[0] == cls]
    print("\n%s: %d" % (cls, len(sel)))
    for r in sel:
        print("  %s consensus crc %d allele %s %s: library (nm, unmapped) %s port %s" % r[1:])
ctx.close()

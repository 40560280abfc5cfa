"""The cost of the ties pass (SP_HLA_MAP_TIES) and of the flags = 0 path against the parent commit: ONE map_consensus_batch call over the four configs[1] consensuses,
15 timed runs after warm-up, wall clock around the call (it ends in a device synchronise).

usage: hla_ties_cost.py run ROOT          one process on the library of the checkout ROOT (this one, or a tree of the parent commit with its library built):
                                          prints one JSON line {"root", "ties": has the library the flag, "plain": [ms x 15], "with_ties": [ms x 15] | null, "k2_ties_ms": ...}
       hla_ties_cost.py compare PARENT    alternates fresh processes parent / this / parent / this and prints the report kept in profiles/hla_map/ties.txt"""
import gzip, json, os, subprocess, sys, time, zlib

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
RUNS, WARM = 15, 3


def run(root):
    sys.path.insert(0, root)
    import __graft_entry__ as ge
    pkg = ge.load_package()
    from pb_starphase_amd import synth
    gold = json.load(gzip.open(os.path.join(root, "tests", "golden", "concordance.json.gz"), "rt"))
    ctx = pkg.Context(0)
    fx = synth.HlaFixture(); db = fx.make_db(pkg, ctx)
    items, pairs = [], 0
    for row in gold["k2"]["consensuses"]:
        gi = fx.genes.index(row["gene"])
        cons = [c for c in gold["hla"]["consensus"][row["gene"]] if zlib.crc32(c.encode()) & 0xFFFFFFFF == row["consensus_crc"]][0]
        m = db.map_type_consensus(gi, cons)
        items.append((gi, m.cons_dna, m.cons_cdna)); pairs += len(m.alleles)
    has = hasattr(pkg.ffi, "SP_HLA_MAP_TIES")
    L = pkg.ffi.lib()
    import ctypes as C
    import numpy as np
    n = len(items)
    g = np.array([it[0] for it in items], np.uint32)
    d = (C.c_char_p * n)(*[it[1].encode() for it in items]); dl = np.array([len(it[1]) for it in items], np.uint32)
    c = (C.c_char_p * n)(*[it[2].encode() for it in items]); cl = np.array([len(it[2]) for it in items], np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(ties):
        """the C call alone (the Python reader of the handle copies every CIGAR, which is not the library's time); the handle is freed outside the clock"""
        h = C.c_void_p()
        t = time.perf_counter()
        if ties:
            rc = L.sp_hla_map_consensus_batch_ex(ctx._h, db._h, n, ptr(g), d, ptr(dl), c, ptr(cl), 0, 0, 1, C.byref(h))
        else:
            rc = L.sp_hla_map_consensus_batch(ctx._h, db._h, n, ptr(g), d, ptr(dl), c, ptr(cl), 0, 0, C.byref(h))
        ms = (time.perf_counter() - t) * 1e3
        assert rc == 0
        L.sp_hla_map_free(h)
        return ms
    for _ in range(WARM):
        call(False)
        if has:
            call(True)
    plain, with_ties = [], []
    ctx.profile_reset()
    for _ in range(RUNS):                                   # alternating, so that a drift of the machine meets both
        plain.append(call(False))
        if has:
            with_ties.append(call(True))
    out = {"root": root, "ties": has, "plain": plain, "with_ties": with_ties if has else None, "pairs": pairs}
    if has:
        out["k2_ties_gpu_ms_per_call"] = [ctx.profile_get(k)[0] / RUNS for k in ("k2_ties", "k2_ties_mm2")]
        out["k2_scan_gpu_ms_per_call"] = [ctx.profile_get(k)[0] / (2 * RUNS) for k in ("k2_scan", "k2_scan_mm2")]
    print("RESULT " + json.dumps(out))
    ctx.close()


def stat(v):
    v = sorted(v)
    return "median %.3f  min %.3f  max %.3f" % (v[len(v) // 2], v[0], v[-1])


def compare(parent):
    res = []
    for who, root in (("parent", parent), ("this", HERE), ("parent", parent), ("this", HERE)):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "run", root], capture_output=True, text=True, timeout=280)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(who, "failed:", p.stderr[-2000:]); sys.exit(1)
        res.append((who, json.loads(line[0][7:])))
    print("one sp_hla_map_consensus_batch call, the four configs[1] consensuses (%d candidate pairs per level), wall ms around the C call; %d runs after %d warm-up calls;" % (res[0][1]["pairs"], RUNS, WARM))
    print("four fresh processes in turn: parent commit, this commit, parent, this")
    for who, r in res:
        print("%-6s flags = 0   : %s" % (who, stat(r["plain"])))
        if r["ties"]:
            print("%-6s with ties   : %s" % (who, stat(r["with_ties"])))
            print("%-6s GPU ms per call: k2_ties %.4f, k2_ties_mm2 %.4f (k2_scan %.4f, k2_scan_mm2 %.4f)" % ((who,) + tuple(r["k2_ties_gpu_ms_per_call"]) + tuple(r["k2_scan_gpu_ms_per_call"])))
    par = sorted(x for who, r in res if who == "parent" for x in r["plain"])
    for who, r in res:
        if who == "this":
            med = sorted(r["plain"])[RUNS // 2]
            print("this flags = 0 median %.3f ms against the parent's own spread over its %d runs, min %.3f - max %.3f: %s" % (med, len(par), par[0], par[-1], "inside" if par[0] <= med <= par[-1] else "OUTSIDE"))
            cost = sorted(r["with_ties"])[RUNS // 2] - med
            print("cost of the pass (median with ties - median without, same process): %.3f ms = %.2f %% of the call" % (cost, 100.0 * cost / med))
    print("raw runs:")
    for who, r in res:
        print(" ", who, "flags = 0:", " ".join("%.3f" % x for x in r["plain"]))
        if r["ties"]:
            print(" ", who, "with ties:", " ".join("%.3f" % x for x in r["with_ties"]))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(os.path.abspath(sys.argv[2]))
    elif len(sys.argv) == 3 and sys.argv[1] == "compare":
        compare(os.path.abspath(sys.argv[2]))
    else:
        sys.exit(__doc__)

"""K5 times for profiles/k5/alternatives.txt: sp_cyp_best_chain_pair (rank 1) and, where the library has it, sp_cyp_best_chain_pairs with N = 10, on
  sample     the chain problem of a 2,000-read synthetic locus (a workgroup per pair)
  tile_edge  a 513-read locus with six CYP2D6 alleles and inference: thousands of pairs, a thread per pair (k5_block_pairs = 0)
Wall time per call on a warm context, `--reps` calls each, rank 1 and N = 10 alternating; min / median / max in ms, one JSON line.

usage: python profiles/scripts/k5_alternatives_perf.py [--package DIR] [--reps 40]
  --package DIR   a tree whose pb-starphase_amd (built) is measured instead of this one's -- the parent commit, for the same-session comparison"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    args = sys.argv[1:]
    tree = args[args.index("--package") + 1] if "--package" in args else ROOT
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 40
    sys.path.insert(0, os.path.abspath(tree))
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    import cyp_cases
    import oracle_ffi as of
    ctx = pkg.Context(0)
    has_n = hasattr(ctx, "cyp_best_chain_pairs")

    def problem(n_d6, n_reads, infer, seed):
        labels, obs, sc, inf = cyp_cases.synthetic_problem(np.random.default_rng(seed), n_d6=n_d6, n_reads=n_reads, noise=0.15, infer=infer)
        inp = of.ChainInputs(labels, obs, sc, inf, True, of.DEFAULT_PENALTIES, False)
        return (inp.types, inp.subtypes, inp.cfg["translate"], inp.cfg["connections"], inp.cfg["singletons"], inp.read_chain_off, inp.chain_off, inp.chain_items,
                inp.read_w_off, inp.w_ed, inp.w_ov, inp.infer, inp.normalize_all, inp.ignore, inp.penalties)

    out = {"package": os.path.abspath(tree), "reps": reps, "n_best": has_n}
    for name, a, limit in (("sample", problem(4, 2000, True, 7), 4096), ("tile_edge", problem(6, 513, True, 5), 0)):
        ctx.set_option("k5_block_pairs", limit)
        rc, res = ctx.cyp_best_chain_pair(*a)
        n_pairs = res.n_possible * (res.n_possible + 1) // 2
        for _ in range(5):
            ctx.cyp_best_chain_pair(*a)
            if has_n:
                ctx.cyp_best_chain_pairs(*a, n=10)
        t1, tn = [], []
        for _ in range(reps):
            t0 = time.perf_counter(); ctx.cyp_best_chain_pair(*a); t1.append((time.perf_counter() - t0) * 1e3)
            if has_n:
                t0 = time.perf_counter(); ctx.cyp_best_chain_pairs(*a, n=10); tn.append((time.perf_counter() - t0) * 1e3)
        e = {"status": rc, "chains": res.n_possible, "pairs": n_pairs, "route": "workgroup" if n_pairs <= limit else "thread",
             "rank1_ms": [round(min(t1), 4), round(statistics.median(t1), 4), round(max(t1), 4)]}
        if has_n:
            e["n10_ms"] = [round(min(tn), 4), round(statistics.median(tn), 4), round(max(tn), 4)]
            for k in ("k5_pairs", "k5_alt_pairs", "k5_alt_select", "k5_alt_coverage"):
                try:
                    ms, launches, cells = ctx.profile_get(k)
                    e[k] = [round(ms, 4), launches]
                except Exception:
                    pass
        out[name] = e
    ctx.set_option("k5_block_pairs", 4096)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

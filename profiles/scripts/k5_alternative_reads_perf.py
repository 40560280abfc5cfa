"""Times for profiles/k5/alternative_reads.txt: sp_cyp_chain_pair_reads on the ten best pairs of the chain problem of a 2,000-read synthetic locus (the `sample`
problem of k5_alternatives_perf.py), and the whole-sample call on the files of tests/test_gpu_diplotype_files.py with sp_starphase_set_cyp_alternative_reads off
and on, alternating.  Wall ms on a warm context, min / median / max; GPU time per launch from sp_profile_get.  One JSON line.

usage: python profiles/scripts/k5_alternative_reads_perf.py [--reps 40] [--calls 6] [--kernel-only] [--keep FILE]
  --kernel-only   the chain_pair_reads calls alone (for a kernel trace of their own)
  --keep FILE     also copy the switch's cyp2d6_alternative_reads.json to FILE"""
import json
import os
import pathlib
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def three(t):
    return [round(min(t), 4), round(statistics.median(t), 4), round(max(t), 4)]


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 40
    calls = int(args[args.index("--calls") + 1]) if "--calls" in args else 6
    keep = args[args.index("--keep") + 1] if "--keep" in args else None
    sys.path.insert(0, ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    import cyp_cases
    import oracle_ffi as of
    ctx = pkg.Context(0)
    labels, obs, sc, inf = cyp_cases.synthetic_problem(np.random.default_rng(7), n_d6=4, n_reads=2000, noise=0.15, infer=True)
    inp = of.ChainInputs(labels, obs, sc, inf, True, of.DEFAULT_PENALTIES, False)
    a = (inp.types, inp.subtypes, inp.cfg["translate"], inp.cfg["connections"], inp.cfg["singletons"], inp.read_chain_off, inp.chain_off, inp.chain_items,
         inp.read_w_off, inp.w_ed, inp.w_ov, inp.infer, inp.normalize_all, inp.ignore, inp.penalties)
    rc, alts, _, _, best = ctx.cyp_best_chain_pairs(*a, n=10)
    which = [(x.index1, x.index2) for x in alts]
    out = {"reps": reps, "status": rc, "chains": best.n_possible, "pairs_asked": len(which), "reads": len(inp.score_names)}
    for _ in range(5):
        ctx.cyp_chain_pair_reads(*a, pairs=which)
    t_with, t_without, t_n10 = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter(); ctx.cyp_chain_pair_reads(*a, pairs=which); t_with.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); ctx.cyp_chain_pair_reads(*a, pairs=which, totals=False); t_without.append((time.perf_counter() - t0) * 1e3)
        if "--kernel-only" not in args:
            t0 = time.perf_counter(); ctx.cyp_best_chain_pairs(*a, n=10); t_n10.append((time.perf_counter() - t0) * 1e3)
    out["pair_reads_ms"], out["pair_reads_no_totals_ms"] = three(t_with), three(t_without)
    if t_n10:
        out["n10_ms"] = three(t_n10)
    for k in ("k5_pair_reads", "k5_pair_reads_totals", "k5_chain_reads"):
        try:
            ms, launches, cells = ctx.profile_get(k)
            out[k] = [round(ms, 4), launches]
        except Exception:
            pass
    if "--kernel-only" in args:
        print(json.dumps(out))
        return
    from test_gpu_diplotype_files import Sample
    root = pathlib.Path(tempfile.mkdtemp())
    sample = Sample(root, pkg)
    handles = {"off": pkg.database.Starphase(sample.db, sample.fasta, debug_folder=str(root / "off")),
               "on": pkg.database.Starphase(sample.db, sample.fasta, debug_folder=str(root / "on"), cyp_alternative_reads=True),
               "both": pkg.database.Starphase(sample.db, sample.fasta, debug_folder=str(root / "both"), cyp_alternative_reads=True, cyp_alternatives=True)}
    times = {k: [] for k in handles}
    for k, h in handles.items():
        for _ in range(2):
            h.call(bams=sample.bams, vcf=sample.vcf)
    for _ in range(calls):
        for k, h in handles.items():
            t0 = time.perf_counter(); h.call(bams=sample.bams, vcf=sample.vcf); times[k].append((time.perf_counter() - t0) * 1e3)
    for k, h in handles.items():
        out["sample_%s_ms" % k] = three(times[k])
        h.close()
    if keep:
        shutil.copy(root / "on" / "cyp2d6_alternative_reads.json", keep)
    shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

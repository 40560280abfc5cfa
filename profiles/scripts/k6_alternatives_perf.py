"""Times for profiles/k6/alternatives.txt: sp_variant_solve_batch and sp_variant_alternatives_batch (N = 10) on a panel-shaped batch (23 problems x 32 samples,
random problems of the shape of tests/test_gpu_variant.py with 20 .. 100 haplotypes), one problem with 16 unphased hets, and the whole-sample call on the files of
tests/test_gpu_diplotype_files.py with sp_starphase_set_variant_alternatives off and on, alternating.  Wall ms on a warm context, min / median / max; GPU time per
launch from sp_profile_get.  One JSON line.

usage: python profiles/scripts/k6_alternatives_perf.py [--reps 30] [--calls 6] [--root DIR]
  --root DIR   time the tree at DIR instead of this one (a checkout of the parent commit, built: only what that tree has is timed)"""
import json
import os
import pathlib
import shutil
import statistics
import sys
import tempfile
import time


def three(t):
    return [round(min(t), 4), round(statistics.median(t), 4), round(max(t), 4)]


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 30
    calls = int(args[args.index("--calls") + 1]) if "--calls" in args else 6
    root_dir = os.path.abspath(args[args.index("--root") + 1]) if "--root" in args else os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, root_dir)
    sys.path.insert(1, os.path.join(root_dir, "tests"))
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    from test_gpu_variant import RandomProblem, gpu_struct
    ctx = pkg.Context(0)
    has_alt = hasattr(ctx, "variant_alternatives_batch")
    rng = np.random.default_rng(5)
    probs = [RandomProblem(rng, n_vars=24, n_haps=int(rng.integers(20, 101)), n_obs=int(rng.integers(0, 11))) for _ in range(23 * 32)]
    structs = [gpu_struct(pkg, p) for p in probs]
    out = {"tree": root_dir, "reps": reps, "problems": len(structs)}
    for _ in range(3):
        ctx.variant_solve_batch(structs)
        if has_alt:
            ctx.variant_alternatives_batch(structs, 10)
    t_solve, t_alt = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); ctx.variant_solve_batch(structs); t_solve.append((time.perf_counter() - t0) * 1e3)
        if has_alt:
            t0 = time.perf_counter(); got = ctx.variant_alternatives_batch(structs, 10); t_alt.append((time.perf_counter() - t0) * 1e3)
    out["panel_solve_ms"] = three(t_solve)
    if has_alt:
        out["panel_alternatives_ms"] = three(t_alt)
        out["panel_candidates"] = int(sum(g[0].n_candidates for g in got))
        out["panel_assignments"] = int(sum(g[0].n_comb for g in got))
        # one problem with 16 unphased hets (32,768 assignments) and 60 haplotypes
        big = RandomProblem(rng, n_vars=24, n_haps=60, n_obs=16)
        big.obs_gt[:] = 1; big.obs_ps[:] = -1; big.obs_sv[:] = -1
        s = gpu_struct(pkg, big)
        t_big, t_big_solve = [], []
        for k in range(3 + min(reps, 10)):
            t0 = time.perf_counter(); info, _alts = ctx.variant_alternatives(s, 10); t1 = time.perf_counter(); ctx.variant_solve(s); t2 = time.perf_counter()
            if k >= 3:
                t_big.append((t1 - t0) * 1e3); t_big_solve.append((t2 - t1) * 1e3)
        out["hets16_alternatives_ms"], out["hets16_solve_ms"] = three(t_big), three(t_big_solve)
        out["hets16_assignments"], out["hets16_candidates"] = int(info.n_comb), int(info.n_candidates)
    for k in ("k6_cells", "k6_alt", "k6_alt_select"):
        try:
            ms, launches, _cells = ctx.profile_get(k)
            out[k] = [round(ms, 4), launches]
        except Exception:
            pass
    from test_gpu_diplotype_files import Sample
    root = pathlib.Path(tempfile.mkdtemp())
    sample = Sample(root, pkg)
    handles = {"off": pkg.database.Starphase(sample.db, sample.fasta, debug_folder=str(root / "off"))}
    if has_alt:
        handles["on"] = pkg.database.Starphase(sample.db, sample.fasta, debug_folder=str(root / "on"), variant_alternatives=True)
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
    shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

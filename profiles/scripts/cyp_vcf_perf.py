"""What cyp2d6_alleles.vcf.gz costs (DESIGN.md sections 7.2 and 10), on the device this runs on, for one configs[2] sample (*4+*68/*1, 2,000 reads):
  1. the member pass of sp_cyp_consensus_support without windows, three rounds of REPS warm calls (median, min-max): the figure a parent commit's run of the same
     call is to be held against, by its own min-max spread
  2. sp_cyp_variant_support with the table (the same pass with the windows attached, behind the backbone alignments): wall, and the kernels' time from the profile
  3. the whole switch: 2. plus rendering and saving the file
The parent commit itself is not run by this script.
usage: python profiles/scripts/cyp_vcf_perf.py [out.txt]"""
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402

REPS = 9
CONS_CAP = 65536
KERNELS = ("anchor", "affine_align", "align_pileup_map", "align_pileup_pile", "align_pileup_summary", "pileup_windows")


def timed(fn, reps=REPS):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    out = []
    say = lambda s="": (out.append(s), print(s, flush=True))
    pkg = ge.load_package()
    import cyp_cases_real as cr
    from pb_starphase_amd import synth
    D, ffi = pkg.database, pkg.ffi
    ctx = pkg.Context(0)
    cfg, gene_def = cr.load_db()
    locus = synth.Chr22Locus(cfg, gene_def, seed=3)
    cdb = ffi.CypDb(ctx, cfg, gene_def, locus.sequence, locus.start)
    haps, _truth = {n: (h, e) for n, h, e in cr.scenarios(locus)}["*4+*68/*1"]
    reads = locus.sample(np.random.default_rng(7), haps, 2000)
    R = ctx.upload(reads)
    pr, call, cons, rv, mappings = D.cyp_call_with_variants(cdb, R, CONS_CAP)
    typed = [h for h in range(call.n_consensus) if rv.has_variants[h] == 1]
    plain = lambda: D.cyp_consensus_support(ctx, R, call, cons, CONS_CAP, mappings)
    with_windows = lambda: D.cyp_variant_support(ctx, pr, R, call, cons, CONS_CAP, rv, mappings, table=True)
    sup, ok, _tab = with_windows()
    say(f"one configs[2] sample (*4+*68/*1, {len(reads)} reads): {len(mappings)} members on {call.n_consensus} consensuses, {len(typed)} of them typed, "
        f"{int(ok.sum())} windows of {int(pr.n_variants)} variants x {len(typed)} regions (flank {D.SP_CYP_VCF_FLANK})")
    for k in range(3):
        m = timed(plain)
        say(f"1. member pass without windows, round {k + 1}: wall median {m[0]:.2f} ms, min-max {m[1]:.2f}-{m[2]:.2f} ms ({REPS} warm calls)")
    m = timed(with_windows)
    say(f"2. sp_cyp_variant_support with the table: wall median {m[0]:.2f} ms, min-max {m[1]:.2f}-{m[2]:.2f} ms")
    for name, fn in (("without windows", plain), ("with windows", with_windows)):
        ctx.profile_reset()
        fn()
        say(f"   kernels, {name}: " + ", ".join(f"{k} {ctx.profile_get(k)[0]:.3f} ms x{ctx.profile_get(k)[1]}" for k in KERNELS))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cyp2d6_alleles.vcf.gz")

        def whole():
            s, o, _t = with_windows()
            D.cyp_alleles_vcf_save(cdb, call, rv, path, support=s, support_valid=o)
        m = timed(whole)
        say(f"3. the whole switch (backbone alignments + pass + file of {os.path.getsize(path):,} bytes): wall median {m[0]:.2f} ms, min-max {m[1]:.2f}-{m[2]:.2f} ms")
    say("the parent commit was not run beside it: not measured")
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()

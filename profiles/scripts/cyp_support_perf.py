"""The three figures of DESIGN.md section 7.2 for the CYP2D6 consensus support, on the device this runs on:
  1. sp_align_pileup_batch against sp_affine_align_batch(64, 4096) + sp_pileup_batch on the (segment, consensus) pairs of one configs[2] sample
     (*4+*68/*1, 2,000 reads): wall time of the calls (median of REPS warm calls), kernel time from the context's profile, bytes copied each way (counted from the
     arrays the two routes move)
  2. a whole-sample call (the files of tests/test_gpu_diplotype_files.py: 95 HLA + 120 CYP2D6 reads) with the switch off: median and spread of REPS warm calls, in two
     rounds that alternate with the switch-on rounds; the figures an earlier commit recorded for the same call (profiles/batch/refactor_branch_*.json) are printed
     beside them as read from those files.  The parent commit itself is not run by this script
  3. the same call with the switch on: what the switch adds per sample
usage: python profiles/scripts/cyp_support_perf.py [out.txt]"""
import json
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


def timed(fn, reps=REPS):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def kernel_ms(ctx, names, fn):
    ctx.profile_reset()
    fn()
    return {n: ctx.profile_get(n)[0] for n in names}


def main():
    out = []
    say = lambda s="": (out.append(s), print(s, flush=True))
    pkg = ge.load_package()
    import cyp_cases_real as cr
    from pb_starphase_amd import synth
    D, ffi = pkg.database, pkg.ffi
    ctx = pkg.Context(0)
    # ---- 1. the pairs of one sample
    cfg, gene_def = cr.load_db()
    locus = synth.Chr22Locus(cfg, gene_def, seed=3)
    cdb = ffi.CypDb(ctx, cfg, gene_def, locus.sequence, locus.start)
    haps, _truth = {n: (h, e) for n, h, e in cr.scenarios(locus)}["*4+*68/*1"]
    reads = locus.sample(np.random.default_rng(7), haps, 2000)
    R = ctx.upload(reads)
    call, cons, mappings = D.cyp_call_with_consensus(cdb, R, CONS_CAP)
    text = [D.cyp_consensus_of(cons, CONS_CAP, h) for h in range(call.n_consensus)]
    live = [h for h in range(len(text)) if text[h]]
    members = [m for m in mappings if m.consensus in live]
    queries = [reads[m.read][m.read_start:m.read_end] for m in members]
    target = [live.index(m.consensus) for m in members]
    T, Q = ctx.upload([text[h] for h in live]), ctx.upload(queries)
    diag, votes = ctx.anchor_batch(T, Q, target, list(range(len(queries))))
    pairs = [(m, target[m], -int(diag[m]), 0 if votes[m] > 0 else -1) for m in range(len(queries))]
    n, n_cols = len(pairs), sum(len(text[h]) for h in live)
    say(f"1. one configs[2] sample (*4+*68/*1, {len(reads)} reads): {n} pairs on {len(live)} consensuses, {n_cols} columns, {sum(map(len, queries))} query bases")

    def composition():
        aln, cigar, n_cigar = ctx.affine_align(Q, T, pairs, a=1, band=64, cigar_stride=4096)
        return ctx.pileup(Q, T, pairs, aln, cigar, n_cigar), n_cigar

    resident = lambda: ctx.align_pileup(Q, T, pairs)
    summaries_only = lambda: ctx.align_pileup(Q, T, pairs, aln=False, cols=False)
    _tabs, n_cigar = composition()
    ops = int(n_cigar.sum())
    k_comp = kernel_ms(ctx, ("affine_align", "pileup"), composition)
    k_res = kernel_ms(ctx, ("align_pileup_map", "align_pileup_pile", "align_pileup_summary"), resident)
    w_comp, w_res, w_sum = timed(composition), timed(resident), timed(summaries_only)
    say(f"   composition   wall {w_comp[0]:8.2f} ms (min {w_comp[1]:.2f}, max {w_comp[2]:.2f}; the Python binding's array handling included)   kernels " +
        ", ".join(f"{k} {v:.2f} ms" for k, v in k_comp.items()))
    say(f"   resident      wall {w_res[0]:8.2f} ms (min {w_res[1]:.2f}, max {w_res[2]:.2f})   kernels " + ", ".join(f"{k} {v:.2f} ms" for k, v in k_res.items()))
    say(f"   resident, summaries only   wall {w_sum[0]:8.2f} ms (min {w_sum[1]:.2f}, max {w_sum[2]:.2f})")
    pair_b, aln_b, col_b = 16 * n, 24 * n, 32 * n_cols
    down_comp = aln_b + 4 * n + 4 * 4096 * n + col_b
    up_comp = 2 * pair_b + 8 * n + 24 * n + 4 * ops                                   # pairs twice, scratch offsets, the pileup's pair records, the ops again
    say(f"   bytes   composition: up {up_comp:,} down {down_comp:,} (rows of 4,096 ops: {4 * 4096 * n:,}; {ops:,} ops in use)")
    say(f"           resident:    up {pair_b + 4 * n + 8 * (len(live) + 1):,} down {aln_b + col_b + 32 * len(live):,} (aln + table + summaries); summaries only: down {32 * len(live):,}")
    # ---- 2. / 3. the whole-sample call
    from test_gpu_diplotype_files import Sample
    import pathlib
    with tempfile.TemporaryDirectory() as tmp:
        sample = Sample(pathlib.Path(tmp), pkg)
        dbg = os.path.join(tmp, "dbg")
        h = D.Starphase(sample.db, sample.fasta, debug_folder=dbg)
        kw = dict(bams=sample.bams, vcf=sample.vcf)
        res = {}
        for _round in range(2):                                                       # off, on, off, on: both see the same machine
            for on in (False, True):
                h.set_cyp_consensus_support(on)
                res.setdefault(on, []).append(timed(lambda: h.call(**kw)))
        h.close()
    off = [r[0] for r in res[False]]
    on = [r[0] for r in res[True]]
    say(f"2. whole-sample call, switch off: medians of {REPS} warm calls {off[0]:.2f} / {off[1]:.2f} ms, min-max {min(r[1] for r in res[False]):.2f}-{max(r[2] for r in res[False]):.2f} ms")
    earlier = []
    for k in (1, 2, 3):                                                               # the same call as an earlier commit recorded it, where those records exist
        path = os.path.join(ROOT, "profiles", "batch", f"refactor_branch_{k}.json")
        if os.path.exists(path):
            earlier.append(json.load(open(path))["single_steady_call_ms_median"])
    say("   (the parent commit was not run beside it" + (f"; steady single call on the same files as recorded for an earlier commit, profiles/batch/refactor_branch_*.json: "
        + " / ".join(f"{v:.2f}" for v in earlier) + " ms)" if earlier else ")"))
    say(f"3. switch on: medians {on[0]:.2f} / {on[1]:.2f} ms, min-max {min(r[1] for r in res[True]):.2f}-{max(r[2] for r in res[True]):.2f} ms: "
        f"+{statistics.mean(on) - statistics.mean(off):.2f} ms per sample (120 CYP2D6 reads)")
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()

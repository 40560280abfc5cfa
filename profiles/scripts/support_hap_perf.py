"""What the haplotype list (sp_support_hap) costs, and whether the pass is unchanged without it, by the method of cyp_support_perf.py:
  1. the (segment, consensus) pairs of one configs[2] sample (*4+*68/*1, 2,000 reads): the device-resident pass (Context.align_pileup) without and with the list,
     alternating, REPS warm calls each in one process; raw figures, medians, the list's launches from the context's profile, what a cold context's first call did
  2. the HLA support call (HlaDb.consensus_support on the synthetic fixture of tests/test_gpu_consensus_support.py, both genes) the same way
  2b. the HLA support call on the 10,000-read sample of BASELINE configs[1] (synth.Config2Workload, every gene; about 2,500 members per consensus, so a gene's
     batch crosses SP_ALIGN_PILEUP_SLICE and a target's sort leaves LDS), with each gene's consensus 1 edited as tests/test_gpu_support_hap.py edits it (three bases
     deleted, one changed 40 further on) so that contested columns exist and the list has work to do
  3. the pass WITHOUT the list in a process of its own, on this tree and -- with --parent-tree DIR, a built checkout of the parent commit -- on the parent's, one after
     the other, ROUNDS times in turn in the same session: "unchanged" means this tree's median lies inside the parent's own min-max spread
usage: python profiles/scripts/support_hap_perf.py [out.txt] [--parent-tree DIR]        (the child processes: --tree DIR --only-without)"""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ARGS = sys.argv[1:]
HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def option(name):
    return ARGS[ARGS.index(name) + 1] if name in ARGS else None


ROOT = os.path.abspath(option("--tree") or HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402

REPS = 5
ROUNDS = 2
CONS_CAP = 65536


def ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def alternate(without, with_list, reps=REPS):
    """one warm-up each, then without / with in turn: both see the same machine"""
    without()
    with_list()
    a, b = [], []
    for _ in range(reps):
        a.append(ms(without))
        b.append(ms(with_list))
    return a, b


def fmt(ts):
    return " ".join(f"{t:.2f}" for t in ts) + f"   median {statistics.median(ts):.2f}, min-max {min(ts):.2f}-{max(ts):.2f} ms"


def cyp_pairs(pkg, ctx):
    import cyp_cases_real as cr
    from pb_starphase_amd import synth
    D, ffi = pkg.database, pkg.ffi
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
    return Q, T, pairs, sum(map(len, queries))


def hla_call(pkg, ctx):
    from pb_starphase_amd import synth
    fx = synth.HlaFixture(max_alleles_per_gene=40, seed=7)
    db = fx.make_db(pkg, ctx)
    rng = np.random.default_rng(11)
    fwd = [g for g in range(len(fx.genes)) if fx.gene_fwd[g] and fx.full_length_alleles(g)][0]
    rev = [g for g in range(len(fx.genes)) if not fx.gene_fwd[g] and fx.full_length_alleles(g)][0]
    reads = []
    for g, n in ((fwd, 9), (rev, 14)):
        a = fx.full_length_alleles(g)[0]
        hap, s = fx.haplotype(g, a)
        reads += synth.simulate_reads(rng, hap, s, len(fx.dna[a]), n, mean_len=6000, sd_len=800)
    R = ctx.upload(reads)
    rec = db.realign_reads(R)
    genes = [fwd, rev]
    out, is1 = db.diplotype_genes(genes, R, rec)
    return db, genes, R, rec, is1, out


def gap_site(s, lo):
    """the first p >= lo at which s[p:p + 3], deleted, can be put back at one place only (tests/test_gpu_support_ins.py)"""
    for p in range(lo, len(s) - 4):
        if s[p] != s[p + 3] and s[p + 2] != s[p - 1]:
            return p
    raise AssertionError("no site")


def hla10k_call(pkg, ctx):
    from pb_starphase_amd import synth
    fx = synth.HlaFixture()
    db = fx.make_db(pkg, ctx)
    wl = synth.Config2Workload(fx, n_reads=10000, seed=1000)
    R = ctx.upload(wl.reads)
    rec = db.realign_reads(R)
    genes = list(range(len(fx.genes)))
    out, is1 = db.diplotype_genes(genes, R, rec)
    swap = {"A": "C", "C": "G", "G": "T", "T": "A"}
    cons = []
    for call, c1, c2 in out:
        p = gap_site(c1, len(c1) // 2)
        cut = c1[:p] + c1[p + 3:]
        cons.append((cut[:p + 40] + swap[cut[p + 40]] + cut[p + 41:], c2))
    return db, genes, R, rec, is1, cons


def main():
    out = []
    say = lambda s="": (out.append(s), print(s, flush=True))
    pkg = ge.load_package()
    ctx = pkg.Context(0)
    Q, T, pairs, q_bases = cyp_pairs(pkg, ctx)
    db, genes, R, rec, is1, calls = hla_call(pkg, ctx)
    cyp_without = lambda: ctx.align_pileup(Q, T, pairs)
    hla_without = lambda: [db.consensus_support(g, R, rec, is1, calls[k][1], calls[k][2]) for k, g in enumerate(genes)]
    db2, genes2, R2, rec2, is12, cons2 = hla10k_call(pkg, ctx)
    big_without = lambda: [db2.consensus_support(g, R2, rec2, is12, cons2[k][0], cons2[k][1]) for k, g in enumerate(genes2)]
    if "--only-without" in ARGS:
        # a child process: the pass without the list alone, REPS warm calls each (this tree or the parent's)
        res = {}
        for name, fn in (("cyp", cyp_without), ("hla", hla_without), ("hla10k", big_without)):
            fn()
            res[name] = [ms(fn) for _ in range(REPS)]
        print("RESULT " + json.dumps(res), flush=True)
        return
    say(f"1. one configs[2] sample (*4+*68/*1, 2,000 reads): {len(pairs)} pairs, {q_bases} query bases; Context.align_pileup, {REPS} warm calls each, alternating")
    cold = ms(lambda: ctx.align_pileup(Q, T, pairs, haplotypes=True))
    haps, heads = ctx.align_pileup(Q, T, pairs, haplotypes=True)[3]
    say(f"   the list: {len(haps)} records over {int((heads['n_records'] > 0).sum())} targets, {int(heads['n_cols'].sum())} columns used of {int(heads['n_cols_total'].sum())} contested; "
        f"first call on this context {cold:.2f} ms")
    a, b = alternate(cyp_without, lambda: ctx.align_pileup(Q, T, pairs, haplotypes=True))
    say("   without the list  " + fmt(a))
    say("   with the list     " + fmt(b))
    say(f"   the list adds {statistics.median(b) - statistics.median(a):+.2f} ms (medians)")
    ctx.profile_reset()
    ctx.align_pileup(Q, T, pairs, haplotypes=True)
    names = ("align_pileup_map", "align_pileup_pile", "align_pileup_summary", "support_hap")
    say("   kernels of one call with the list: " + ", ".join(f"{n} {ctx.profile_get(n)[0]:.3f} ms" for n in names))
    say(f"2. the HLA support call (HlaDb.consensus_support, two genes, {int((rec['status'] == 0).sum())} member reads), {REPS} warm calls each, alternating")
    a, b = alternate(hla_without, lambda: [db.consensus_support(g, R, rec, is1, calls[k][1], calls[k][2], haplotypes=True) for k, g in enumerate(genes)])
    say("   without the list  " + fmt(a))
    say("   with the list     " + fmt(b))
    say(f"   the list adds {statistics.median(b) - statistics.median(a):+.2f} ms (medians)")
    say(f"2b. the HLA support call on the 10,000-read sample ({len(genes2)} genes, {int((rec2['status'] == 0).sum())} member reads, consensus 1 of each gene edited), {REPS} warm calls each, alternating")
    big_with = lambda: [db2.consensus_support(g, R2, rec2, is12, cons2[k][0], cons2[k][1], haplotypes=True) for k, g in enumerate(genes2)]
    for k, res in enumerate(big_with()):
        (cols1, sm1), (cols2, sm2), (haps, heads) = res
        say(f"   gene {k}: members {sm1['n_members']} + {sm2['n_members']}, aligned {sm1['n_aligned']} + {sm2['n_aligned']}; contested columns {[int(x) for x in heads['n_cols_total']]}, "
            f"used {[int(x) for x in heads['n_cols']]}; {len(haps)} records, largest patterns {[int(x) for x in haps['count'][:4]]}")
    a, b = alternate(big_without, big_with)
    say("   without the list  " + fmt(a))
    say("   with the list     " + fmt(b))
    say(f"   the list adds {statistics.median(b) - statistics.median(a):+.2f} ms (medians) to {len(genes2)} calls")
    ctx.profile_reset()
    big_with()
    names2 = ("consensus_support_map", "consensus_support_map_retry", "pileup", "consensus_support_summary", "support_hap")
    say("   kernels of the calls with the list: " + ", ".join(f"{n} {ctx.profile_get(n)[0]:.3f} ms / {ctx.profile_get(n)[1]} launches" for n in names2))
    say(f"3. the pass without the list in a process of its own, {REPS} warm calls, the trees in turn, {ROUNDS} rounds")
    trees = [("this tree", HERE)] + ([("parent commit", os.path.abspath(option("--parent-tree")))] if option("--parent-tree") else [])
    got = {}
    for label, tree in trees * ROUNDS:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", tree, "--only-without"], capture_output=True, text=True, timeout=1500)
        line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            say(f"   {label}: the child process failed ({p.returncode}): {p.stderr[-300:]}")
            continue
        res = json.loads(line[-1][7:])
        for name in ("cyp", "hla", "hla10k"):
            say(f"   {label:14s} {name}  " + fmt(res[name]))
            got.setdefault(label, {}).setdefault(name, []).extend(res[name])
    if len(got) == 2:
        for name in ("cyp", "hla", "hla10k"):
            mine, par = statistics.median(got["this tree"][name]), got["parent commit"][name]
            inside = min(par) <= mine <= max(par)
            say(f"   {name}: this tree's median {mine:.2f} ms is {'inside' if inside else 'OUTSIDE'} the parent's min-max spread {min(par):.2f}-{max(par):.2f} ms"
                + ("" if inside else f" (by {mine - (max(par) if mine > max(par) else min(par)):+.2f} ms)"))
    else:
        say("   (no parent tree was given: the parent commit was not run)")
    target = [x for x in ARGS if not x.startswith("--") and x not in (option("--tree"), option("--parent-tree"))]
    if target:
        os.makedirs(os.path.dirname(os.path.abspath(target[0])), exist_ok=True)
        open(target[0], "w").write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()

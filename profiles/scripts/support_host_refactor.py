"""The host side of consensus support (csrc/sp_support.hip) against another build of the library: the same device work, the same results, the same wall time.
One process per library, the libraries in turn, ROUNDS times in one session.  Each process builds the two-gene HLA call of tests/test_gpu_consensus_support.py and
the two CYP2D6 samples of tests/test_gpu_cyp_support.py, edits a consensus of each as tests/test_gpu_support_hap.py does (so that both lists have records), and for
HlaDb.consensus_support_cohort and database.cyp_consensus_support_cohort, with both lists and with neither:
  - warms the call up twice, then takes from the context's profile what ONE call launches (launches, cells per name) and what it adds to pool:device,
  - times REPS further calls (wall clock; every call ends in a stream synchronise),
  - hashes everything the call returned.
usage: python profiles/scripts/support_host_refactor.py OUT.txt --other PATH/libstarphase_hip.so        (the child processes: --child)"""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))

REPS = 10
ROUNDS = 4
CONS_CAP = 32768
NAMES = ("consensus_support_map", "consensus_support_map_retry", "consensus_support_summary", "pileup", "align_pileup_map", "align_pileup_map_retry", "align_pileup_pile",
         "align_pileup_summary", "pileup_ins_collect", "pileup_ins_reduce", "support_hap", "pool:device")
SWAP = {"A": "C", "C": "G", "G": "T", "T": "A"}


def gap_site(s, lo):
    for p in range(lo, len(s) - 4):
        if s[p] != s[p + 3] and s[p + 2] != s[p - 1]:
            return p
    raise AssertionError("no site")


def edit(text):
    """three bases deleted in the middle, the base 40 further on changed (tests/test_gpu_support_hap.py)"""
    p = gap_site(text, len(text) // 2)
    cut = text[:p] + text[p + 3:]
    return cut[:p + 40] + SWAP[cut[p + 40]] + cut[p + 41:]


def digest(x, h):
    if isinstance(x, np.ndarray):
        h.update(x.tobytes())
    elif isinstance(x, dict):
        h.update(json.dumps(x, sort_keys=True).encode())
    elif x is not None:
        for y in x:
            digest(y, h)


def child():
    import ctypes as C
    import __graft_entry__ as ge
    import cyp_fixture as cf
    import oracle_ffi as of
    pkg = ge.load_package()
    from pb_starphase_amd import synth
    ctx = pkg.Context(0)
    D = pkg.database
    # the HLA call
    fx = synth.HlaFixture(max_alleles_per_gene=40, seed=7)
    db = fx.make_db(pkg, ctx)
    rng = np.random.default_rng(11)
    genes = [[g for g in range(len(fx.genes)) if fx.gene_fwd[g] == fwd and fx.full_length_alleles(g)][0] for fwd in (True, False)]
    reads = []
    for g, n in zip(genes, (9, 14)):
        a = fx.full_length_alleles(g)[0]
        hap, s = fx.haplotype(g, a)
        reads += synth.simulate_reads(rng, hap, s, len(fx.dna[a]), n, mean_len=6000, sd_len=800)
    R = ctx.upload(reads)
    rec = db.realign_reads(R)
    out, is1 = db.diplotype_genes(genes, R, rec)
    cons = [[(edit(c1), c2) for _call, c1, c2 in out]]
    # the CYP2D6 samples
    locus = synth.CypLocus(seed=11)
    cdb, d6 = cf.make_db(locus, synth, np.random.default_rng(5))
    templates = ctx.upload(cdb.seqs)
    problem = ctx.cyp_problem(templates, cdb.types, cdb.subtypes, cdb.deep, cdb.backbone, cdb.variants, cdb.is_vi, cdb.allele_subtypes, cdb.hap_matrix, of.default_cyp_config())
    sets, calls, blocks, maps = [], [], [], []
    for scenario in ("*1/*4", "*4x2/*1"):
        S = ctx.upload(cf.sample(locus, synth, np.random.default_rng(7), d6, scenario, 120))
        call, block, mappings = D.cyp_problem_call_with_consensus(ctx, problem, S, CONS_CAP)
        raw = bytearray(block.raw)
        text = D.cyp_consensus_of(block, CONS_CAP, 0)
        raw[:CONS_CAP] = edit(text).encode().ljust(CONS_CAP, b"\0")
        sets.append(S), calls.append(call), blocks.append(C.create_string_buffer(bytes(raw), len(raw))), maps.append(mappings)
    cases = {
        "hla, both lists": lambda: db.consensus_support_cohort(1, None, genes, R, rec, is1, cons, insertions=True, haplotypes=True),
        "hla, no list": lambda: db.consensus_support_cohort(1, None, genes, R, rec, is1, cons),
        "cyp, both lists": lambda: D.cyp_consensus_support_cohort(ctx, sets, calls, blocks, CONS_CAP, maps, insertions=True, haplotypes=True),
        "cyp, no list": lambda: D.cyp_consensus_support_cohort(ctx, sets, calls, blocks, CONS_CAP, maps),
    }
    res = {}
    for name, fn in cases.items():
        fn()
        fn()
        before = {n: ctx.profile_get(n)[1:] for n in NAMES}
        got = fn()
        now = {n: ctx.profile_get(n)[1:] for n in NAMES}
        h = hashlib.sha256()
        digest(got, h)
        ms = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        res[name] = dict(one_call={n: [now[n][0] - before[n][0], now[n][1] - before[n][1]] for n in NAMES}, sha=h.hexdigest()[:16], ms=ms)
    res["pool:device at the end"] = list(ctx.profile_get("pool:device")[1:])
    print("RESULT " + json.dumps(res))


def main():
    out_path, other = sys.argv[1], os.path.abspath(sys.argv[sys.argv.index("--other") + 1])
    runs = {"this tree": [], "other library": []}
    for _ in range(ROUNDS):
        for who in ("other library", "this tree"):
            env = dict(os.environ)
            env.pop("SP_LIB_PATH", None)
            if who == "other library":
                env["SP_LIB_PATH"] = other
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=400)
            line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.exit(f"{who}: exit status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
            runs[who].append(json.loads(line[0][7:]))
    lines = []
    first = runs["other library"][0]
    for case in [k for k in first if k != "pool:device at the end"]:
        lines.append(case)
        same = all(r[case]["one_call"] == first[case]["one_call"] and r[case]["sha"] == first[case]["sha"] for rs in runs.values() for r in rs)
        lines.append(f"   one warm call, (launches, cells) per profile name, the same in every process of both libraries: {same}; results' sha256 prefix {first[case]['sha']}")
        lines.append("      " + ", ".join(f"{n} {tuple(v)}" for n, v in first[case]["one_call"].items() if v != [0, 0] or n == "pool:device"))
        for who, rs in runs.items():
            for k, r in enumerate(rs):
                lines.append(f"   {who:13s} round {k + 1}  " + " ".join(f"{t:.2f}" for t in r[case]["ms"]) + f"   min-max {min(r[case]['ms']):.2f}-{max(r[case]['ms']):.2f} ms")
        mine = [t for r in runs["this tree"] for t in r[case]["ms"]]
        theirs = [t for r in runs["other library"] for t in r[case]["ms"]]
        inside = max(mine) <= max(theirs)
        lines.append(f"   this tree {min(mine):.2f}-{max(mine):.2f} ms, the other library {min(theirs):.2f}-{max(theirs):.2f} ms: "
                     + ("inside the other's spread or on its fast side" if inside else f"OUTSIDE on the slow side by {max(mine) - max(theirs):+.2f} ms"))
    lines.append("pool:device (allocations, bytes) at the end of each process: " + "; ".join(f"{who} {[tuple(r['pool:device at the end']) for r in rs]}" for who, rs in runs.items()))
    text = "\n".join(lines) + "\n"
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()

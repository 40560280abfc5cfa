"""K5 with one workgroup per pair (k5_pair_block_kernel): sp_cyp_best_chain_pair on a synthetic locus of 2,000 reads whose few thousand chain pairs stay
under k5_block_pairs' default; the k5_pairs and k5_chain_reads device times of each of N warm calls, their median and their spread.
Run on the GPU box:  python profiles/scripts/k5_block_speed.py [calls]     (SP_LIB_PATH names another build to compare with, in a process of its own)"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_package()
import cyp_cases
import oracle_ffi as of
from test_gpu_cyp import gpu_chain_pair


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 25
    labels, obs, sc, infer = cyp_cases.synthetic_problem(np.random.default_rng(3), n_d6=3, n_reads=2000, noise=0.15, infer=True)
    inp = of.ChainInputs(labels, obs, sc, infer, True, of.DEFAULT_PENALTIES, False)
    ctx = pkg.Context(0)
    pairs_ms, tab_ms = [], []
    for k in range(3 + calls):                                   # three calls to warm up
        ctx.profile_reset()
        rc, res = gpu_chain_pair(ctx, inp)
        ctx.synchronize()
        if k >= 3:
            pairs_ms.append(ctx.profile_get("k5_pairs")[0]); tab_ms.append(ctx.profile_get("k5_chain_reads")[0])
    P = res.n_possible
    rec = {"lib": pkg.lib_path(), "reads": 2000, "chains_P": P, "pairs": P * (P + 1) // 2, "pairs_scored": int(res.n_pairs_scored), "status": rc, "calls": calls,
           "k5_pairs_ms_median": statistics.median(pairs_ms), "k5_pairs_ms_min": min(pairs_ms), "k5_pairs_ms_max": max(pairs_ms),
           "k5_chain_reads_ms_median": statistics.median(tab_ms), "score": res.score, "index": [res.index1, res.index2]}
    print(json.dumps(rec), flush=True)


main()

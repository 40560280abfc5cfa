"""sp_cyp_chain_pair_reads (k5_pair_reads_kernel) and sp_cyp_observed_chains through the C ABI, held to tests/chain_pair_reads_ref.py field for field; the records
explain sp_cyp_best_chain_pairs' scores (edit_distance, unmet_observations, hap_weights bit for bit) on both routes of k5_block_pairs; any pair can be asked for."""
import numpy as np
import pytest

import chain_pair_reads_ref as rref
import chain_pairs_ref as ref
import cyp_cases
import oracle_ffi as of
from chain_pair_reads_cases import chains_of, hand_made, problem
from test_gpu_cyp import gpu_chain_pair
from test_gpu_cyp_alternatives import bits, call_args, graph_problem, pairs, path, pruning_problem, ref_problems, routes

gpu = pytest.mark.gpu
FIELDS = ("mask1", "mask2", "excess_ed", "n_best", "supported")


def reads_of(ctx, inp, which, totals=True):
    return ctx.cyp_chain_pair_reads(*call_args(inp), pairs=which, totals=totals)


def all_pairs(chains, n=None):
    out = [(i, j) for i in range(len(chains)) for j in range(i, len(chains))]
    if n is not None:                                                      # any list of pairs may be asked for: the list repeated up to n
        out = [out[k % len(out)] for k in range(n)]
    return out


def same_records(got, want, what=""):
    assert got.shape == (len(want), len(want[0]) if want else 0), (what, got.shape)
    for f in FIELDS:
        w = np.array([[rec[f] for rec in row] for row in want], np.uint64).reshape(got.shape)
        g = got[f].astype(np.uint64)
        bad = np.argwhere(g != w)
        assert not len(bad), "%s: %s differs at (pair, read) %s: %s, expected %s" % (what, f, tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])])
    assert not got["reserved_"].any()


def check(ctx, inp, chains, which, what=""):
    rc, recs, ed, un = reads_of(ctx, inp, which)
    assert rc == 0, what
    want = rref.pair_reads(inp, chains, which)
    same_records(recs, want, what)
    assert [int(v) for v in ed] == [sum(rec["excess_ed"] for rec in row) for row in want], what      # the optional totals are the column sums
    assert [int(v) for v in un] == [sum(1 - rec["supported"] for rec in row) for row in want], what
    return recs, want


def long_path(H=40):
    """a path of H regions, label limits ignored: the chain 0 .. H-1 is enumerated, and read `z` fits it best at start 35 -- the upper half of the mask"""
    obs, sc = {}, {}
    for k, (a, b) in enumerate(path(H)):
        obs["e%04d" % k] = [[a, b]]
        sc["e%04d" % k] = [[(0 if x == a else 3, 1.0) for x in range(H)], [(0 if x == b else 3, 1.0) for x in range(H)]]
    obs["z"] = [[35]]
    sc["z"] = [[(0 if x == 35 else 2, 0.5) for x in range(H)]]
    return of.ChainInputs([("CYP2D6", str(h + 1)) for h in range(H)], obs, sc, False, True, of.DEFAULT_PENALTIES, True)


@gpu
def test_records_at_the_block_edge(pkg, gpu_ctx):
    """check 1: R = 1, 255, 256, 257 reads with n_pairs = 1 and 64 (homozygous pairs among them)"""
    rng = np.random.default_rng(41)
    for R in (1, 255, 256, 257):
        inp = graph_problem(rng, 4, path(4), R - 3, max_len=2) if R > 1 else graph_problem(rng, 2, [(0, 1)], 0)
        assert len(inp.score_names) == R
        chains = chains_of(pkg, inp)
        many = all_pairs(chains, 64)
        assert any(i == j for i, j in many)
        for limit in routes(gpu_ctx):
            check(gpu_ctx, inp, chains, many[-1:], "R %d, one pair" % R)
            recs, want = check(gpu_ctx, inp, chains, many, "R %d, 64 pairs" % R)
        for k, (i, j) in enumerate(many):
            if i == j:
                assert np.array_equal(recs["mask1"][k], recs["mask2"][k])
                assert np.array_equal(recs["n_best"][k], 2 * np.array([bin(int(m)).count("1") for m in recs["mask1"][k]]))


@gpu
def test_records_of_the_designed_reads(pkg, gpu_ctx):
    """check 1: a read longer than both chains, longer than one, without observed chains, without weight rows; every start a best one; ties between the chains"""
    inp = hand_made()
    chains = chains_of(pkg, inp)
    assert sorted(chains) == [[0], [0, 1], [1], [2]]
    which = all_pairs(chains)
    recs, want = check(gpu_ctx, inp, chains, which, "hand_made")
    names = sorted(["edge", "long", "noobs", "norows", "two"])
    r_long, r_noobs, r_norows = names.index("long"), names.index("noobs"), names.index("norows")
    k_short = which.index(tuple(sorted((chains.index([0]), chains.index([2])))))
    k_one = which.index(tuple(sorted((chains.index([0, 1]), chains.index([2])))))
    optimum, worst = 1 + 1, 4 + 7
    q = recs[k_short][r_long]                                                       # longer than both chains: no placement
    assert (int(q["n_best"]), int(q["mask1"]), int(q["mask2"]), int(q["excess_ed"])) == (0, 0, 0, 2 * worst - optimum)
    q = recs[k_one][r_long]                                                         # longer than [2] only: start 0 of [0, 1], total 1 + 1
    assert int(q["n_best"]) == 1 and int(q["mask1"]) + int(q["mask2"]) == 1 and int(q["excess_ed"]) == 0
    assert not recs["supported"][:, r_noobs].any()                                   # `any` over nothing
    for k, (i, j) in enumerate(which):                                               # no weight rows: every start 0 .. len of both chains, nothing above the optimum
        q = recs[k][r_norows]
        assert (int(q["mask1"]), int(q["mask2"]), int(q["excess_ed"])) == ((2 << len(chains[i])) - 1, (2 << len(chains[j])) - 1, 0)
        assert int(q["supported"]) == (1 if 1 in chains[i] + chains[j] else 0)
    every = ref_problems()["many_addends"]                                           # all_equal_read: every start of every chain
    chains = chains_of(pkg, every)
    which = all_pairs(chains)[:64]
    recs, want = check(gpu_ctx, every, chains, which, "many_addends")
    r0 = sorted(every.score_names).index("r00000")
    for k, (i, j) in enumerate(which):
        if len(chains[i]) >= 2 and len(chains[j]) >= 2:
            assert int(recs[k][r0]["n_best"]) == len(chains[i]) - 1 + len(chains[j]) - 1
    twins = graph_problem(np.random.default_rng(11), 4, [(0, 1), (0, 2), (1, 3), (2, 3)], 30, dup=(1, 2))
    chains = chains_of(pkg, twins)
    which = all_pairs(chains)[:64]
    recs, want = check(gpu_ctx, twins, chains, which, "dup")
    assert ((recs["mask1"] != 0) & (recs["mask2"] != 0) & (recs["mask1"] != recs["mask2"])).any()      # a read that ties between two different chains


def test_a_long_path_enumerates_a_chain_with_starts_past_32(pkg):
    """(CPU) with the label limits ignored a path of 40 regions enumerates the chain 0 .. 39"""
    chains = chains_of(pkg, long_path())
    assert list(range(40)) in chains and len(chains) == 40 * 41 // 2


@gpu
def test_the_upper_half_of_the_mask(pkg, gpu_ctx):
    """check 1: a best start at position 32 or beyond"""
    inp = long_path()
    chains = chains_of(pkg, inp)
    full, tail = chains.index(list(range(40))), chains.index([38, 39])
    which = [(full, full), tuple(sorted((full, tail))), (min(full, 0), max(full, 0))]
    recs, want = check(gpu_ctx, inp, chains, which, "long_path")
    z = sorted(inp.score_names).index("z")
    assert int(recs[0][z]["mask1"]) == 1 << 35 and int(recs[0][z]["excess_ed"]) == 0
    assert (recs["mask1"] >> np.uint64(32)).any() and (recs["mask2"] >> np.uint64(32)).any()


def explain_cases():
    return list(ref_problems().items()) + [(name, inp) for name, inp, _, _, _ in cyp_cases.reference_cases()]


@gpu
def test_the_records_explain_the_scores(pkg, gpu_ctx):
    """check 2: for the ten best pairs, the column sums are edit_distance and unmet_observations, and hap_weights recomputed from the masks is sp_cyp_best_chain_pairs'
    bit for bit -- on both routes"""
    seen = 0
    for name, inp in explain_cases():
        for limit in routes(gpu_ctx):
            rc, alts, counts, weights, best = pairs(gpu_ctx, inp, 10)
            which = [(a.index1, a.index2) for a in alts] or [(0, 0)]
            rc2, recs, ed, un = reads_of(gpu_ctx, inp, which)
            if rc != 0:
                assert rc2 == rc == gpu_chain_pair(gpu_ctx, inp)[0], name                   # the expected failures of the enumeration
                continue
            assert rc2 == 0, name
            chains = chains_of(pkg, inp)
            for k, a in enumerate(alts):
                assert int(recs["excess_ed"][k].sum(dtype=np.uint64)) == a.edit_distance == int(ed[k]), (name, limit, k)
                assert int((recs["supported"][k] == 0).sum()) == a.unmet_observations == int(un[k]), (name, limit, k)
                got = rref.hap_weights(inp, chains, which[k], recs[k])
                assert [bits(v) for v in got] == [bits(v) for v in weights[k]], (name, limit, k, got, list(weights[k]))
            rc3, recs3, ed3, un3 = reads_of(gpu_ctx, inp, which, totals=False)
            assert rc3 == 0 and ed3 is None and un3 is None and recs3.tobytes() == recs.tobytes()
            seen += 1
    assert seen >= 2 * (len(ref_problems()) + 6)


@gpu
def test_a_pair_outside_the_top_ten(pkg, gpu_ctx):
    """check 3: a pair the rank-1 bound prunes and a pair get_multinomial_score rejects, both by index"""
    inp = pruning_problem()
    chains = chains_of(pkg, inp)
    want = ref.score_pairs(inp, chains)
    pruned = next(w for w in want[1:] if w["partial_cost"] > want[0]["score"])
    valid = {(w["index1"], w["index2"]) for w in want}
    rejected = next(p for p in all_pairs(chains) if p not in valid)                    # (chains too short for any read: zero rounded coverage)
    which = [(pruned["index1"], pruned["index2"]), rejected, (want[0]["index1"], want[0]["index2"])]
    for limit in routes(gpu_ctx):
        recs, w = check(gpu_ctx, inp, chains, which, "pruning_problem")
    assert int(recs["excess_ed"][0].sum()) == pruned["edit_distance"] and int((recs["supported"][0] == 0).sum()) == pruned["unmet_observations"]
    assert [bits(v) for v in rref.hap_weights(inp, chains, which[0], recs[0])] == [bits(v) for v in pruned["hap_weights"]]
    assert sum(round(v) for v in rref.hap_weights(inp, chains, rejected, recs[1])) == 0


@gpu
def test_argument_errors(pkg, gpu_ctx):
    """check 4"""
    inp = hand_made()
    P = len(chains_of(pkg, inp))
    for bad in ([(0, P)], [(P, P)], [(-1, 0)], [(1, 0)], [(0, 0), (2, 1)], [], [(0, 0)] * 65):
        with pytest.raises(pkg.StarphaseError) as e:
            reads_of(gpu_ctx, inp, bad)
        assert e.value.code == pkg.ffi.SP_ERR_INVALID_ARG, bad
    assert reads_of(gpu_ctx, inp, [(0, 0)] * 64)[0] == 0
    failing = [(name, inp, status) for name, inp, status, _, _ in cyp_cases.reference_cases() if status != 0]
    assert failing
    for name, inp, status in failing:
        assert reads_of(gpu_ctx, inp, [(0, 0)])[0] == gpu_chain_pair(gpu_ctx, inp)[0] == status, name


@gpu
def test_a_warm_call_allocates_nothing(pkg, gpu_ctx):
    """check 5: a second identical call adds no device allocation ("pool:device")"""
    inp = ref_problems()["H12"]
    which = all_pairs(chains_of(pkg, inp))[:10]
    for limit in routes(gpu_ctx):
        first = reads_of(gpu_ctx, inp, which)
        before = gpu_ctx.profile_get("pool:device")
        second = reads_of(gpu_ctx, inp, which)
        after = gpu_ctx.profile_get("pool:device")
        assert before[1] == after[1], (before, after)
        assert first[1].tobytes() == second[1].tobytes()


def several_chains_per_read():
    """reads with 1, 2 and 3 observed chains: weights 1, 1/2 and 1/3, so the order of the additions shows in the last bit"""
    rng = np.random.default_rng(77)
    menu = [[0, 1], [0, 2], [1, 2], [0, 1, 2], [2], [1, 2, 3], [3]]
    obs = {}
    for r in range(60):
        n = int(rng.integers(1, 4))
        obs["r%03d" % r] = [menu[int(k)] for k in rng.choice(len(menu), n, replace=False)]
    return of.ChainInputs([("CYP2D6", str(h + 1)) for h in range(4)], obs, {}, False, True, of.DEFAULT_PENALTIES, True)


def test_observed_chains_equal_the_python_reference(pkg):
    """check 6 (host only): chains, frequencies, node totals, edges and edge totals, f64 bit for bit"""
    cases = list(ref_problems().items()) + [("several", several_chains_per_read())]
    thirds = 0
    for name, inp in cases:
        p, keep = problem(pkg, inp)
        chains, freq, single, edges, weight = pkg.ffi.observed_chains(p)
        w_chains, w_freq, w_single, w_edges, w_weight = rref.observed_table(inp)
        assert chains == w_chains and edges == w_edges, name
        assert chains == sorted(chains) and edges == sorted(edges)
        for got, want in ((freq, w_freq), (single, w_single), (weight, w_weight)):
            assert [bits(v) for v in got] == [bits(v) for v in want], (name, list(got), want)
        thirds += sum(1 for v in freq if v != round(v * 2) / 2)
    assert thirds                                                                       # (a frequency that is no multiple of 1/2: thirds were added)
    # the counts are always set; a buffer too small is SP_ERR_CAPACITY
    import ctypes as C
    p, keep = problem(pkg, several_chains_per_read())
    nc, ni, ne = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    rc = pkg.ffi.lib().sp_cyp_observed_chains(None, C.byref(p), None, 0, None, 0, None, None, None, None, None, 0, C.byref(nc), C.byref(ni), C.byref(ne))
    table = rref.observed_table(several_chains_per_read())
    assert rc == pkg.ffi.SP_ERR_CAPACITY and (nc.value, ni.value, ne.value) == (len(table[0]), sum(len(c) for c in table[0]), len(table[3]))

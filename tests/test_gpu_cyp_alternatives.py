"""sp_cyp_best_chain_pairs (K5's N-best mode) through the C ABI: entry 0 is sp_cyp_best_chain_pair's call, the pruning is exact, the list is ordered and
complete, and -- with the label limits ignored -- it equals tests/chain_pairs_ref.py bit for bit; a warm call allocates nothing.

The number of pairs is triangular (P (P + 1) / 2), so the thread kernel's block edge is met at 253 pairs (P = 22: one block, three idle lanes -- every valid
pair of the problem sits in one 256-thread block, which must emit N of them) and 276 pairs (P = 23: a second block of 20 pairs); 255 / 256 / 257 do not exist."""
import struct

import numpy as np
import pytest

import chain_pairs_ref as ref
import cyp_cases
import oracle_ffi as of
from test_gpu_cyp import gpu_chain_pair

pytestmark = pytest.mark.gpu

FIELDS = ("score", "ln_ed_penalty", "mn_llh_penalty", "allele_expected_penalty", "unexpected_chain_penalty", "inferred_chain_penalty")
ROUTES = (0, 1 << 20)                                        # k5_block_pairs: a thread per pair, a workgroup per pair


def bits(x):
    return struct.pack("<d", float(x))


def call_args(inp):
    n_reads = max(len(inp.chain_names), len(inp.score_names))
    rco = inp.read_chain_off if len(inp.read_chain_off) == n_reads + 1 else np.zeros(n_reads + 1, np.int32)
    rwo = inp.read_w_off if len(inp.read_w_off) == n_reads + 1 else np.zeros(n_reads + 1, np.int32)
    return (inp.types, inp.subtypes, inp.cfg["translate"], inp.cfg["connections"], inp.cfg["singletons"], rco, inp.chain_off, inp.chain_items, rwo,
            inp.w_ed, inp.w_ov, inp.infer, inp.normalize_all, inp.ignore, inp.penalties)


def pairs(ctx, inp, n):
    return ctx.cyp_best_chain_pairs(*call_args(inp), n=n)


def key(a):
    return (bits(a.score), a.index1, a.index2, a.n1, a.n2, list(a.chain1[:a.n1]), list(a.chain2[:a.n2]), tuple(bits(getattr(a, f)) for f in FIELDS),
            a.edit_distance, a.unmet_observations)


def check_order(alts):
    ks = [(a.score, a.index1, a.index2) for a in alts]
    assert all(x < y for x, y in zip(ks, ks[1:])), ks                    # strictly ascending: ordered and distinct
    assert all(a.index1 <= a.index2 for a in alts)


class routes:
    def __init__(self, ctx):
        self.ctx = ctx

    def __iter__(self):
        try:
            for limit in ROUTES:
                self.ctx.set_option("k5_block_pairs", limit)
                yield limit
        finally:
            self.ctx.set_option("k5_block_pairs", 4096)


def graph_problem(rng, H, edges, n_reads, max_len=3, lasso=4.0, ln_ed=2.0, types=None, all_equal_read=False, dup=None):
    """A problem with the label limits ignored and no inference: the observed chains of the reads carry `edges`; a read sees a window of a random walk along the
    edges with small random edit distances (ties are common) and random overlaps (so the order of the f64 sums matters).  dup = (a, b): region b is a copy of
    region a (same columns).  all_equal_read: the first read scores every region alike over two positions, so every window of every chain is a best one (more
    than eight addends)."""
    labels = types or [("CYP2D6", str(h + 1)) for h in range(H)]
    nxt = {h: [b for a, b in edges if a == h] for h in range(H)}
    obs, sc = {}, {}
    for k, (a, b) in enumerate(edges):                                    # every edge is observed, whatever the reads below draw
        obs["e%04d" % k] = [[a, b]]
        sc["e%04d" % k] = [[(0 if x == a else 3, 1.0) for x in range(H)], [(0 if x == b else 3, 1.0) for x in range(H)]]
    for r in range(n_reads):
        walk = [int(rng.integers(H))]
        while len(walk) < int(rng.integers(1, max_len + 1)) and nxt[walk[-1]]:
            walk.append(nxt[walk[-1]][int(rng.integers(len(nxt[walk[-1]])))])
        rows = []
        for h in walk:
            row = [(0 if x == h else int(rng.integers(0, 4)), float(rng.random())) for x in range(H)]
            if dup:
                row[dup[1]] = row[dup[0]]
            rows.append(row)
        if all_equal_read and r == 0:
            walk = walk[:1] * 2
            rows = [[(1, float(rng.random())) for x in range(H)] for _ in range(2)]
        obs["r%05d" % r] = [walk]
        sc["r%05d" % r] = rows
    return of.ChainInputs(labels, obs, sc, False, True, (lasso, ln_ed, 10.0, 2.0), True)


def path(H, start=0):
    return [(h, h + 1) for h in range(start, H - 1)]


def ref_list(gpu_ctx, inp):
    rc, chains = gpu_ctx.cyp_possible_chains(*call_args(inp))
    assert rc == 0
    return chains, ref.score_pairs(inp, chains)


def same_as_ref(alts, counts, weights, want):
    assert len(alts) == len(want)
    for k, (a, w) in enumerate(zip(alts, want)):
        assert (a.index1, a.index2) == (w["index1"], w["index2"]), (k, a.index1, a.index2, w["index1"], w["index2"])
        assert a.edit_distance == w["edit_distance"] and a.unmet_observations == w["unmet_observations"], k
        assert list(counts[k]) == w["hap_counts"], k
        for f in FIELDS:
            assert bits(getattr(a, f)) == bits(w[f]), (k, f, getattr(a, f), w[f])
        assert [bits(v) for v in weights[k]] == [bits(v) for v in w["hap_weights"]], (k, list(weights[k]), w["hap_weights"])


def entry0_cases(oracle):
    out = [(name, inp, of.oracle_chain_pair(oracle, inp)) for name, inp, status, _, _ in cyp_cases.reference_cases()]
    for n_reads in (1, 2, 255, 256, 257, 513):                            # the generator of test_gpu_cyp.py::test_chain_pair_kernels_at_tile_edges
        for noise in (0.0, 0.15):
            for infer in (False, True):
                labels, obs, sc, inf = cyp_cases.synthetic_problem(np.random.default_rng(5), n_d6=3, n_reads=n_reads, noise=noise, infer=infer)
                inp = of.ChainInputs(labels, obs, sc, inf, True, of.DEFAULT_PENALTIES, False)
                out.append(("edge_%d_%s_%d" % (n_reads, noise, infer), inp, of.oracle_chain_pair(oracle, inp)))
    return out


def test_entry_0_is_the_call(oracle, gpu_ctx):
    """check 1: for N in {1, 10}, on both routes, entry 0 and `best` equal sp_cyp_best_chain_pair and the oracle field for field, f64 bit for bit"""
    cases = entry0_cases(oracle)
    for limit in routes(gpu_ctx):
        for name, inp, exp in cases:
            rc1, one = gpu_chain_pair(gpu_ctx, inp)
            assert rc1 == exp.status, name
            for n in (1, 10):
                rc, alts, counts, weights, best = pairs(gpu_ctx, inp, n)
                assert rc == exp.status, (name, n, rc)
                if rc != 0:
                    assert not alts
                    continue
                check_order(alts)
                assert 1 <= len(alts) <= n
                a = alts[0]
                for got in (a, best):
                    for other in (one, exp):
                        assert (got.index1, got.index2, got.n1, got.n2) == (other.index1, other.index2, other.n1, other.n2), (name, n, limit)
                        assert list(got.chain1[:got.n1]) == list(other.chain1[:other.n1]) and list(got.chain2[:got.n2]) == list(other.chain2[:other.n2])
                        for f in FIELDS:
                            assert bits(getattr(got, f)) == bits(getattr(other, f)), (name, n, limit, f)
                        assert got.edit_distance == other.edit_distance
                assert best.n_possible == one.n_possible == exp.n_possible
                assert a.unmet_observations == exp.unmet_observations, name


def pruning_problem():
    """Two haplotypes of seven regions each on a path of fourteen (105 chains, 5,565 pairs), two reads per edge of a haplotype; the edge that joins the two is
    observed by one read that fits everywhere.  A wrong region costs 5 edits at 100 each and a second copy of a region costs 200, so the call -- both
    haplotypes, nothing twice, the multinomial term alone -- is followed by pairs that overlap in one or two regions with no edits: their partial cost, 200 or
    400, is above the best complete score -- the rank-1 bound prunes them --, and they are the runners-up."""
    H = 14
    obs, sc = {}, {}
    k = 0
    for a, b in path(7) + path(14, 7):
        for rep in range(2):
            obs["r%03d" % k] = [[a, b]]
            sc["r%03d" % k] = [[(0 if x == a else 5, 1.0) for x in range(H)], [(0 if x == b else 5, 1.0) for x in range(H)]]
            k += 1
    obs["r%03d" % k] = [[6, 7]]
    sc["r%03d" % k] = [[(0, 1.0)] * H, [(0, 1.0)] * H]
    labels = [("CYP2D6", str(h + 1)) for h in range(H)]
    return of.ChainInputs(labels, obs, sc, False, True, (200.0, 100.0, 10.0, 2.0), True)


def test_pruning_is_exact(gpu_ctx):
    """check 2: the N = 10 list is a prefix of the N = 64 list and the first ten of the unpruned list -- the Python reference's, which prunes nothing -- on a
    problem where the rank-1 call demonstrably prunes (n_pairs_scored < n_pairs) and pairs the rank-1 bound prunes belong to the top ten"""
    inp = pruning_problem()
    chains, want = ref_list(gpu_ctx, inp)
    n_pairs = len(chains) * (len(chains) + 1) // 2
    assert n_pairs == 5565 and len(want) > 64
    assert any(w["partial_cost"] > want[0]["score"] for w in want[1:10])          # the case is what it was built to be (checked on the CPU)
    small = graph_problem(np.random.default_rng(3), 4, path(4), 12)             # valid pairs <= 64: the N = 64 call is the unpruned list
    for limit in routes(gpu_ctx):
        rc, ten, c10, w10, best10 = pairs(gpu_ctx, inp, 10)
        rc64, all64, c64, w64, best64 = pairs(gpu_ctx, inp, 64)
        assert rc == 0 and rc64 == 0 and len(ten) == 10 and len(all64) == 64
        check_order(all64)
        assert [key(a) for a in ten] == [key(a) for a in all64[:10]]
        assert np.array_equal(c10, c64[:10]) and w10.tobytes() == w64[:10].tobytes()
        same_as_ref(all64, c64, w64, want[:64])
        if limit:                                                               # a workgroup per pair: late pairs start after the early ones have set the bound
            rc1, one = gpu_chain_pair(gpu_ctx, inp)
            print("rank-1 pairs scored", one.n_pairs_scored, "of", n_pairs, "; N = 10:", best10.n_pairs_scored, "; N = 64:", best64.n_pairs_scored)
            assert rc1 == 0 and one.n_pairs_scored < n_pairs
            assert best10.n_pairs_scored <= n_pairs
        rc, s10, _, _, _ = pairs(gpu_ctx, small, 10)
        rc64, s64, _, _, _ = pairs(gpu_ctx, small, 64)
        assert rc == 0 and rc64 == 0 and len(s64) < 64 and len(s10) == 10
        assert [key(a) for a in s10] == [key(a) for a in s64[:10]]


def test_order_and_count(oracle, gpu_ctx):
    """check 3: strictly ascending (score, index1, index2), distinct pairs, n_alts = min(N, valid pairs): N above the number of valid pairs, exactly one valid
    pair (the reference's *5/*5 scenario), and duplicated regions, whose pairs tie on the score to the last bit so that (i, j) alone orders them"""
    double5 = next(c[1] for c in cyp_cases.reference_cases() if c[0] == "double5")
    twins = graph_problem(np.random.default_rng(11), 4, [(0, 1), (0, 2), (1, 3), (2, 3)], 30, dup=(1, 2))
    chains, want = ref_list(gpu_ctx, twins)
    ties = sum(1 for x, y in zip(want, want[1:]) if bits(x["score"]) == bits(y["score"]))
    assert ties >= 3 and len(want) < 64                                          # (the case is what it was built to be)
    for limit in routes(gpu_ctx):
        rc, alts, _, _, best = pairs(gpu_ctx, double5, 10)
        assert rc == 0 and len(alts) == 1 and (alts[0].index1, alts[0].index2) == (0, 0) and best.n_possible == 1
        for n in (1, 3, 10, 64):
            rc, alts, counts, weights, _ = pairs(gpu_ctx, twins, n)
            assert rc == 0 and len(alts) == min(n, len(want))
            check_order(alts)
            assert len({(a.index1, a.index2) for a in alts}) == len(alts)
            same_as_ref(alts, counts, weights, want[:n])
    with pytest.raises(Exception):
        pairs(gpu_ctx, twins, 0)
    with pytest.raises(Exception):
        pairs(gpu_ctx, twins, 65)


def ref_problems():
    rng = np.random.default_rng(29)
    out = {}
    out["H2_self_loop"] = graph_problem(rng, 2, [(0, 0), (0, 1)], 9)                                   # H = 2, chains with copies: the lasso term
    out["pairs_253"] = graph_problem(rng, 7, path(6), 40)                                              # P = 21 + 1 = 22: 253 pairs, one block of the thread kernel
    out["pairs_276"] = graph_problem(rng, 8, path(6), 40)                                              # P = 23: 276 pairs, a second block of 20
    for R in (1, 256, 257):                                                                            # the K5_TILE edge of the workgroup kernel (3 edge reads + R - 3)
        out["reads_%d" % R] = graph_problem(rng, 4, path(4), R - 3, max_len=2) if R > 1 else graph_problem(rng, 2, [(0, 1)], 0)
    out["many_addends"] = graph_problem(rng, 3, [(0, 0), (0, 1), (1, 2)], 20, all_equal_read=True)      # a read with more than K5_ADDS addends
    out["H12"] = graph_problem(rng, 12, path(12), 30, max_len=4)                                        # as many regions as the synthetic loci of test_gpu_cyp.py; 3,081 pairs
    star5 = [("CYP2D6*5", None), ("CYP2D6", "1"), ("CYP2D6", "2")]
    out["with_deletion"] = graph_problem(rng, 3, [(1, 2)], 10, types=star5)
    return out


@pytest.fixture(scope="module")
def ref_cases(gpu_ctx):
    out = []
    for name, inp in ref_problems().items():
        chains, want = ref_list(gpu_ctx, inp)
        out.append((name, inp, chains, want))
    return out


def test_against_the_python_reference(ref_cases, gpu_ctx):
    """check 4: the N = 10 list equals the reference's first ten bit for bit on both routes -- indices, the five components, score, edit_distance,
    unmet_observations, hap_counts and hap_weights (every quantity turned out bit-reproducible: ln n! past 170 is taken from libm's lgamma, as the library does)"""
    assert {len(c[1].score_names) for c in ref_cases} >= {1, 256, 257}
    assert {len(c[2]) for c in ref_cases} >= {22, 23}
    for limit in routes(gpu_ctx):
        for name, inp, chains, want in ref_cases:
            rc, alts, counts, weights, best = pairs(gpu_ctx, inp, 10)
            assert rc == 0 and best.n_possible == len(chains), name
            assert len(alts) == min(10, len(want)), (name, len(alts), len(want))
            check_order(alts)
            try:
                same_as_ref(alts, counts, weights, want[:10])
            except AssertionError as e:
                raise AssertionError("%s, k5_block_pairs %d: %s" % (name, limit, e))


def test_a_warm_call_allocates_nothing(ref_cases, gpu_ctx):
    """check 5: a second identical call adds no device allocation ("pool:device")"""
    name, inp, chains, want = next(c for c in ref_cases if c[0] == "H12")
    for limit in routes(gpu_ctx):
        first = pairs(gpu_ctx, inp, 10)
        before = gpu_ctx.profile_get("pool:device")
        second = pairs(gpu_ctx, inp, 10)
        after = gpu_ctx.profile_get("pool:device")
        assert before[1] == after[1], (before, after)                          # (ms, allocations so far, bytes held)
        assert [key(a) for a in first[1]] == [key(a) for a in second[1]]

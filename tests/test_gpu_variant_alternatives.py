"""sp_variant_alternatives (K6 N-best): the N best (het assignment, explanation of side 0, explanation of side 1) candidates of a variant problem, held to the
brute force of variant_alternatives_ref.py (the oracle's quant_match on every cell), to sp_variant_solve, and to the reference's scenarios."""
import ctypes as C

import numpy as np
import pytest

import variant_alternatives_ref as ref
import variant_glue as vg
from test_gpu_variant import RandomProblem, gpu_struct
from test_oracle_variant import CASES, SV_CASES

pytestmark = pytest.mark.gpu

NS = (1, 3, 10, 64)
SP_ERR_TOO_LONG = 5
SEED, N_RANDOM = 47, 40


def random_problems(seed=SEED, count=N_RANDOM):
    """Problems of RandomProblem's shape.  The plain generator never leaves a side without an explanation (0 of 480 problems over twelve seeds: a haplotype
    with few slots explains almost everything), so every fourth problem marks its haplotypes of fewer than four slots as SV haplotypes, which the search skips."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        p = RandomProblem(rng, n_vars=24, n_haps=int(rng.integers(3, 60)), n_obs=int(rng.integers(0, 11)))
        if k % 4 == 3:
            p.hap_is_sv = np.array([1 if p.slot_off[h + 1] - p.slot_off[h] < 4 else int(p.hap_is_sv[h]) for h in range(len(p.haps))], np.uint8)
        out.append(p)
    return out


@pytest.fixture(scope="module")
def problems(oracle):
    probs = random_problems()
    return probs, [ref.Brute(oracle, p) for p in probs]


@pytest.fixture(scope="module")
def plain_problems(oracle):
    """the generator of tests/test_gpu_variant.py as it stands, nothing marked"""
    rng = np.random.default_rng(45)
    probs = [RandomProblem(rng, n_vars=24, n_haps=int(rng.integers(3, 60)), n_obs=int(rng.integers(0, 11))) for _ in range(40)]
    return probs, [ref.Brute(oracle, p) for p in probs]


def check(pkg, gpu_ctx, prob, brute, n):
    info, alts = gpu_ctx.variant_alternatives(gpu_struct(pkg, prob), n)
    got = ref.gpu_records(alts)
    assert got == brute.top(n), (n, got[:3], brute.top(3))
    assert info.n_alts == min(n, len(brute.records)) == len(alts)
    assert (info.n_comb, info.n_candidates, info.n_called, tuple(info.best_score)) == (brute.n_comb, brute.n_candidates, brute.n_called, brute.best_score)
    return info, alts


def test_random_problems_against_the_brute_force(pkg, gpu_ctx, problems):
    probs, brutes = problems
    assert sum(b.n_candidates > 10 for b in brutes) * 3 >= len(brutes)
    assert sum(b.sv_sides > 0 for b in brutes) >= 3
    assert sum(b.ineligible_sides > 0 for b in brutes) >= 3
    assert sum(b.n_sides == 1 for b in brutes) >= 3
    assert sum(b.n_candidates < 10 for b in brutes) >= 3
    L = pkg.ffi.lib()
    for k, (p, b) in enumerate(zip(probs, brutes)):
        for n in NS:
            check(pkg, gpu_ctx, p, b, n)
        if b.n_candidates < 10:                    # the unused records are zero
            alts = (pkg.ffi.sp_variant_alt * 10)()
            C.memset(alts, 0xAB, C.sizeof(alts))
            info = pkg.ffi.sp_variant_alt_info()
            s = gpu_struct(pkg, p)
            assert L.sp_variant_alternatives(gpu_ctx._h, C.byref(s), 10, alts, C.byref(info)) == 0
            assert info.n_alts == b.n_candidates < 10
            assert bytes(alts)[info.n_alts * C.sizeof(pkg.ffi.sp_variant_alt):] == bytes((10 - info.n_alts) * C.sizeof(pkg.ffi.sp_variant_alt)), k


def test_plain_random_problems_against_the_brute_force(pkg, gpu_ctx, plain_problems):
    probs, brutes = plain_problems
    assert sum(b.sv_sides > 0 for b in brutes) >= 3 and sum(b.n_sides == 1 for b in brutes) >= 2 and sum(b.n_candidates > 10 for b in brutes) >= 30
    for p, b in zip(probs, brutes):
        for n in NS:
            check(pkg, gpu_ctx, p, b, n)


def hand(n_haps_slots, obs, n_vars=24, core=None, hap_core=None, hap_sv=None):
    """a problem written out: n_haps_slots = per haplotype a list of slots, a slot a list of alternatives (-1: None); obs = [(var, gt, ps, sv label)] in id order"""
    p = RandomProblem.__new__(RandomProblem)
    p.var_list = list(range(n_vars))
    H = len(n_haps_slots)
    p.haps = [{"name": f"h{h}", "core_allele": None if (hap_core is None or hap_core[h]) else "c"} for h in range(H)]
    slot_off, alt_off, alt_var = [0], [0], []
    for slots in n_haps_slots:
        for s in slots:
            alt_var += s
            alt_off.append(len(alt_var))
        slot_off.append(len(alt_off) - 1)
    p.hap_is_sv = np.array(hap_sv if hap_sv is not None else [0] * H, np.uint8) if H else np.zeros(1, np.uint8)
    p.hap_is_core = np.array([1 if h["core_allele"] is None else 0 for h in p.haps] or [0], np.uint8)
    p.slot_off, p.alt_off, p.alt_var = np.array(slot_off, np.int32), np.array(alt_off, np.int32), np.array(alt_var or [0], np.int32)
    p.var_is_core = np.array(core if core is not None else [1] * n_vars, np.uint8)
    p.obs = [o[0] for o in obs]
    p.obs_var = np.array(p.obs or [0], np.int32)
    p.obs_gt = np.array([o[1] for o in obs] or [0], np.int32)
    p.obs_ps = np.array([o[2] for o in obs] or [0], np.int64)
    p.obs_sv = np.array([o[3] for o in obs] or [-1], np.int32)
    return p


def spread_haps(rng, n, n_vars=24):
    return [[[int(v)] for v in rng.choice(n_vars, int(rng.integers(0, 4)), replace=False)] for _ in range(n)]


def edge_problems():
    rng = np.random.default_rng(7)
    core = (rng.random(24) < 0.6).astype(np.uint8).tolist()
    unph = lambda vs: [(v, 1, -1, -1) for v in vs]
    out = {}
    out["70 haplotypes"] = hand(spread_haps(rng, 70), unph([1, 4, 9]) + [(12, 4, -1, -1)], core=core, hap_core=(rng.random(70) < 0.5).tolist())
    out["2 haplotypes"] = hand([[[1]], [[4], [9, -1]]], unph([1, 4]), core=core)
    out["no haplotypes"] = hand([], unph([1, 4]), core=core)
    out["no haplotypes, no hets"] = hand([], [(3, 4, -1, -1)], core=core)
    out["10 unphased hets"] = hand(spread_haps(rng, 40), unph([0, 2, 4, 6, 8, 10, 12, 14, 16, 18]), core=core, hap_core=(rng.random(40) < 0.5).tolist())
    out["one assignment"] = hand(spread_haps(rng, 12), [(2, 2, 100, -1), (5, 3, 100, -1), (7, 4, -1, -1)], core=core)
    out["both sides SV"] = hand(spread_haps(rng, 9), [(2, 2, 100, 0), (5, 3, 100, 1), (6, 3, 100, 1), (7, 2, 100, 2), (9, 4, -1, -1)], core=core)
    # every assignment of three unphased hets scores the same: haplotypes without slots, so each side's score is its number of calls
    out["ties across assignments"] = hand([[], [], []], unph([3, 5, 8]), core=[1] * 24, hap_core=[1, 0, 1])
    # an assignment with a side nothing explains has the smallest total as solve_diplotype compares them: the solve lists no diplotype, candidates exist
    out["unexplained side first"] = hand([[[1], [2]], [[1], [2], [3]]], unph([1, 2]), core=[1] * 24)
    return out


EDGES = edge_problems()
EDGE_BRUTES = {}                                   # filled once by the test that needs them all


@pytest.mark.parametrize("name", sorted(EDGES))
def test_edge_shapes(oracle, pkg, gpu_ctx, name):
    p = EDGES[name]
    b = ref.Brute(oracle, p)
    score, dips = vg.oracle_solve(oracle, p)
    assert (b.best_score, b.n_called) == (score, len(dips))
    if name == "10 unphased hets":
        assert b.n_comb == 512
    if name == "one assignment":
        assert b.n_comb == 1 and b.n_sides == 2
    if name == "both sides SV":
        assert b.records and all(r[3] < 0 and r[4] < 0 for r in b.records)
    if name == "ties across assignments":
        assert len({r[0] for r in b.records}) == 1 and len({r[5] for r in b.records[:12]}) > 1
    if name.startswith("no haplotypes"):
        assert not b.records and b.best_score[1] == ref.MAX
    if name == "unexplained side first":
        assert b.records and b.records[0][0] != b.best_score and b.n_called == 0
    for n in NS:
        check(pkg, gpu_ctx, p, b, n)


@pytest.mark.parametrize("share", (2, 3, 7))
def test_workgroups_that_own_several_assignments(oracle, pkg, gpu_ctx, problems, plain_problems, share):
    """A lone problem gets a workgroup per assignment up to 8 x CUs, so the calls above never take k6_alt_kernel round its grid-stride loop a second time.  Here the
    brute-forced problems sit in a batch with so many others that a problem has `share` workgroups (the header's rule: min(n_comb, max(1, 8 * CUs / P))): a
    workgroup folds assignment after assignment into a full list, prunes against it, and carries its best total and count along.  Every field against the brute force."""
    names = sorted(EDGES)
    if not EDGE_BRUTES:
        EDGE_BRUTES.update({k: ref.Brute(oracle, EDGES[k]) for k in names})
    probs = [EDGES[k] for k in names] + problems[0] + plain_problems[0]
    brutes = [EDGE_BRUTES[k] for k in names] + problems[1] + plain_problems[1]
    structs = [gpu_struct(pkg, p) for p in probs]
    budget = 8 * gpu_ctx.info()["num_cus"]
    P = budget // share
    assert P > len(structs) and max(1, budget // P) == share
    first, n_fill = len(names), len(structs) - len(names)                                                   # the fillers: the random problems again
    batch = structs + [structs[first + k % n_fill] for k in range(P - len(structs))]
    n_comb = [b.n_comb for b in brutes] + [brutes[first + k % n_fill].n_comb for k in range(P - len(structs))]
    assert EDGE_BRUTES["10 unphased hets"].n_comb == 512 > share and sum(b.n_comb > 2 * share for b in brutes) >= (10 if share < 7 else 4)
    assert EDGE_BRUTES["ties across assignments"].n_comb == 4 and EDGE_BRUTES["unexplained side first"].n_comb == 2
    for n in (10, 1, 64):
        gpu_ctx.profile_reset()
        got = gpu_ctx.variant_alternatives_batch(batch, n)
        _ms, launches, workgroups = gpu_ctx.profile_get("k6_alt")
        assert launches == 1 and workgroups == sum(min(c, share) for c in n_comb)                            # wg_count = min(n_comb, share) < n_comb
        for k, b in enumerate(brutes):
            info, alts = got[k]
            assert ref.gpu_records(alts) == b.top(n), (share, n, k)
            assert (info.n_comb, info.n_candidates, info.n_called, tuple(info.best_score), info.n_alts) == (b.n_comb, b.n_candidates, b.n_called, b.best_score,
                                                                                                          min(n, len(b.records))), (share, n, k)
        for k in range(len(structs), P):                                                                     # a filler equals the copy it repeats
            src = first + (k - len(structs)) % n_fill
            assert ref.gpu_records(got[k][1]) == ref.gpu_records(got[src][1])


def held_to_the_solve(pkg, gpu_ctx, prob, n, solved=None):
    s = gpu_struct(pkg, prob)
    score, dips = solved or gpu_ctx.variant_solve(s)
    info, alts = gpu_ctx.variant_alternatives(s, n)
    assert tuple(info.best_score) == score and info.n_called == len(dips)
    if alts:
        assert tuple(alts[0].score) == score
    called = [(a.dip[0], a.dip[1], a.comb) for a in alts if a.flags & pkg.ffi.SP_VAR_ALT_CALLED]
    # the called entries, in list order, are the solve's list in its order: all of it whenever the list reaches past the best total (n_called <= n alone does
    # not say so: the shadowed candidates at the best total take places too), its beginning otherwise
    if len(alts) < n or tuple(alts[-1].score) != score:
        assert called == dips and info.n_called <= n
    else:
        assert called == dips[:len(called)] and len(alts) == n
        shadowed = sum(1 for a in alts if a.flags & pkg.ffi.SP_VAR_ALT_SHADOWED)
        assert len(called) + shadowed == n and (info.n_called > n or shadowed > 0 or called == dips)
    for a in alts:
        if tuple(a.score) != score or a.flags & pkg.ffi.SP_VAR_ALT_CALLED:
            assert not a.flags & pkg.ffi.SP_VAR_ALT_SHADOWED
            continue
        # at the best total and not called: a core allele whose side holds a sub-allele at the same key
        assert a.flags == pkg.ffi.SP_VAR_ALT_SHADOWED
        shadowed = 0
        for side in range(2):
            h = a.dip[side]
            if h < 0 or not prob.hap_is_core[h]:
                continue
            ids = vg.het_split(prob, a.comb)[side]
            for x in range(len(prob.haps)):
                if prob.hap_is_core[x] or prob.hap_is_sv[x]:
                    continue
                rel = dict(pkg.ffi.variant_alt_relations(s, a.comb, side, x))
                key = [sum(1 for v, r in rel.items() if r == want and bool(prob.var_is_core[v]) == c) for want, c in ((3, True), (2, True), (3, False), (2, False))]
                shadowed += key == list(a.side_score[side])
                if key == list(a.side_score[side]):
                    break
        assert shadowed > 0
    return info, alts


def test_against_the_solve(pkg, gpu_ctx, problems):
    probs, _brutes = problems
    for p in probs:
        for n in (3, 10, 64):
            held_to_the_solve(pkg, gpu_ctx, p, n)
    # 14 unphased hets: 8,192 assignments, no brute force
    rng = np.random.default_rng(11)
    big = hand(spread_haps(rng, 50), [(v, 1, -1, -1) for v in range(14)] + [(20, 4, -1, -1)], core=(rng.random(24) < 0.6).astype(np.uint8).tolist(),
               hap_core=(rng.random(50) < 0.5).tolist())
    info, alts = held_to_the_solve(pkg, gpu_ctx, big, 10)
    assert info.n_comb == 8192 and len(alts) == 10
    keys = [(tuple(a.score), a.comb, a.dip[0], a.dip[1]) for a in alts]
    assert keys == sorted(keys) and len(set(keys)) == 10


def names_of(prob, dip):
    return prob.sv_labels[-dip - 2] if dip < 0 else prob.haps[dip]["name"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[1])
def test_reference_scenarios(oracle, pkg, gpu_ctx, case):
    db, vcf, with_ref, dips, _inexact = case
    _g, prob = vg.load_case(oracle, db, vcf, with_ref)
    b = ref.Brute(oracle, prob)
    info, alts = check(pkg, gpu_ctx, prob, b, 64)
    assert info.n_called <= 64
    called = vg.call_gene(oracle, prob, solver=lambda pr: (tuple(info.best_score), [(a.dip[0], a.dip[1], a.comb) for a in alts if a.flags & 1]))
    assert [frozenset(d) if d[0] != d[1] else d for d in called["diplotypes"]] == [frozenset(d) if d[0] != d[1] else d for d in dips]


@pytest.mark.parametrize("case", SV_CASES, ids=lambda c: c[0])
def test_sv_scenarios(oracle, pkg, gpu_ctx, case):
    sv_vcf, dips, _inexact = case
    _g, prob = vg.load_case(oracle, "DPYD-sv-test", "DPYD-sv-test/empty_small.vcf.gz", True, sv_vcf_key=sv_vcf)
    b = ref.Brute(oracle, prob)
    info, alts = check(pkg, gpu_ctx, prob, b, 64)
    called = vg.call_gene(oracle, prob, solver=lambda pr: (tuple(info.best_score), [(a.dip[0], a.dip[1], a.comb) for a in alts if a.flags & 1]))
    assert called["diplotypes"] == dips


def test_batch_equals_singles(pkg, gpu_ctx):
    rng = np.random.default_rng(34)
    probs = [RandomProblem(rng, n_vars=24, n_haps=int(rng.integers(3, 60)), n_obs=int(rng.integers(0, 11))) for _ in range(60)]
    structs = [gpu_struct(pkg, p) for p in probs]
    flat = lambda r: ((r[0].n_comb, r[0].n_candidates, tuple(r[0].best_score), r[0].n_alts, r[0].n_called), ref.gpu_records(r[1]))
    single = [flat(gpu_ctx.variant_alternatives(s, 10)) for s in structs]
    try:
        for streams in (3, 1):
            gpu_ctx.set_option("hla_split_streams", streams)
            assert [flat(r) for r in gpu_ctx.variant_alternatives_batch(structs, 10)] == single
    finally:
        gpu_ctx.set_option("hla_split_streams", 3)
    assert gpu_ctx.variant_alternatives_batch([], 10) == []
    # a problem with 65 observations fails alone
    bad = hand([[[1]]], [(v, 1, -1, -1) for v in range(65)], n_vars=70)
    mixed = structs[:3] + [gpu_struct(pkg, bad)] + structs[3:6]
    got, rcs = gpu_ctx.variant_alternatives_batch(mixed, 10, problem_rc=True)
    assert rcs == [0, 0, 0, SP_ERR_TOO_LONG, 0, 0, 0]
    assert [flat(r) for r in got[:3] + got[4:]] == single[:6] and got[3][0].n_alts == 0 and got[3][1] == []
    with pytest.raises(pkg.StarphaseError):
        gpu_ctx.variant_alternatives_batch(mixed, 10)
    for n in (0, 65):
        with pytest.raises(pkg.StarphaseError):
            gpu_ctx.variant_alternatives(structs[0], n)


def test_relations_of_every_listed_entry(oracle, pkg, gpu_ctx, problems):
    probs, _brutes = problems
    checked = sv = 0
    for p in probs + [EDGES["both sides SV"]]:
        s = gpu_struct(pkg, p)
        _info, alts = gpu_ctx.variant_alternatives(s, 10)
        label_of = {int(p.obs_var[o]): int(p.obs_sv[o]) for o in range(len(p.obs))}
        for a in alts:
            lists = vg.het_split(p, a.comb)
            for side in range(2):
                got = pkg.ffi.variant_alt_relations(s, a.comb, side, a.dip[side])
                if a.dip[side] >= 0:
                    m, mi, e = vg.quant_match(oracle, p, a.dip[side], lists[side])
                    assert got == [(v, 1) for v in m] + [(v, 3) for v in mi] + [(v, 2) for v in e]
                else:                              # the SV short-circuit: the first label explains the side, every further distinct label is unexpected
                    labelled = [v for v in lists[side] if label_of[v] >= 0]
                    assert got[0] == (labelled[0], 1) and -(label_of[labelled[0]] + 2) == a.dip[side]
                    rest = []
                    for v in labelled[1:]:
                        if label_of[v] not in [label_of[x] for x in rest]:
                            rest.append(v)
                    assert got[1:] == [(v, 2) for v in rest]
                    sv += 1
                core = p.var_is_core
                counts = [sum(1 for v, r in got if r == want and bool(core[v]) == c) for want, c in ((3, True), (2, True), (3, False), (2, False))]
                if a.dip[side] < 0:
                    counts = [0, len(got) - 1, 0, 0]           # labels are core variants whatever var_is_core says of the id
                assert counts == list(a.side_score[side])
                checked += 1
    assert checked > 300 and sv > 3

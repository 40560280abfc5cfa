"""The shortcuts of sp_rescore_mappings (af_classify_kernel, sp_affine.hip: the closed form of lone edits, the DP over the rows around the clusters, K1's
ends_only) == oracle/affine.c on designed edits (tests/rescore_cases.py), through sp_affine_rescore_mappings_audit, which also says which route a pair took.
The reference of every assertion is the CPU oracle on the diagonal the audit reports, never another kernel of the library.

Sizes: 360 designed pairs, 9 with an N, 1,500 fuzz pairs; one oracle pass over the fuzz batch measured 1.8 s on 64 diagonals and 4.6 s on 256 (1.5 s for the
designed batch on 256), so each parametrised case below spends a few seconds in the oracle and well under one on the device; the oracle's numbers are kept per
(pair, diagonal, band, a) for the whole module."""
import pytest

import oracle_ffi as of
import rescore_cases as rc

ENDS_KNOB = 64                                   # what K1's second stage passes (sp_hla.hip)
_batches, _encoded, _expected = {}, {}, {}


def batch(name):
    if name not in _batches:
        _batches[name] = {"designed": rc.designed, "with_n": rc.with_n, "fuzz": rc.fuzz}[name]()
    return _batches[name]


def expected(oracle, name, i, k0, band, a):
    """oracle_affine of pair i of a batch, computed once per (pair, diagonal, band, a) of the module"""
    key = (name, i, int(k0), band, a)
    if key not in _expected:
        if (name, i) not in _encoded:
            c = batch(name)[i]
            _encoded[(name, i)] = (oracle.encode(c.target), oracle.encode(c.query))
        t, q = _encoded[(name, i)]
        _expected[key] = of.oracle_affine(oracle, t, q, int(k0), band, a)
    return _expected[key]


def test_the_design_holds_the_clipping_cases(oracle):
    """from the oracle alone (k0 = 0, band 256, a = 1): at least 20 designed pairs are clipped although 16 or more clean bases lie behind the cluster, at least one
    with 24 or more; every long gap keeps a positive score"""
    clipped = []
    for c in batch("designed"):
        if c.family == "cluster behind a clean end":
            s, nm, ts, te, qs, qe = of.oracle_affine(oracle, c.target, c.query, 0, 256, 1)
            assert s > 0
            if (c.place in ("head", "both") and ts > 0) or (c.place in ("tail", "both") and te < len(c.target)):
                clipped.append(c.clean)
        if c.spelled_as_planted:
            # the unit-cost cell spells these clusters as planted -- mismatches where they were put --, so the routes pinned at their boundaries are the cell's too
            _al, ev = oracle.wfa(c.query, c.target, 0, rc.MAX_ED)
            assert [(int(e >> 30), int(e & 0x3FFFFFFF)) for e in ev[:len(c.edits)]] == [(0, p) for p, _k, _n in c.edits] and not ev[len(c.edits):].any()
        if c.family == "long gap":
            for band in c.bands:
                assert of.oracle_affine(oracle, c.target, c.query, -c.diag, band, 1)[0] > 0, (len(c.target), len(c.query), band)
    print("clipped pairs by clean bases:", sorted(clipped))
    assert sum(1 for x in clipped if x >= 16) >= 20
    assert sum(1 for x in clipped if x >= 24) >= 1


class Run:
    """a batch on the device in one orientation: the sets and the pair list"""
    def __init__(self, ctx, name, band, target_is_a):
        self.name, self.band, self.target_is_a = name, band, target_is_a
        self.idx = [i for i, c in enumerate(batch(name)) if band in c.bands]
        cases = [batch(name)[i] for i in self.idx]
        T, Q = ctx.upload([c.target for c in cases]), ctx.upload([c.query for c in cases])
        self.A, self.B = (T, Q) if target_is_a else (Q, T)
        # diag of a pair = b_pos - a_pos; the cases state t_pos - q_pos
        self.pairs = [(k, k, -c.diag if target_is_a else c.diag, c.max_ed) for k, c in enumerate(cases)]
        self.cases = cases

    def audit(self, ctx, a, windows, ends_only):
        return ctx.rescore_mappings_audit(self.A, self.B, self.pairs, a=a, band=self.band, target_is_a=self.target_is_a, events_stride=rc.EVENTS_STRIDE,
                                          windows=windows, ends_only=ends_only)


_runs = {}


def run_of(ctx, name, band, target_is_a):
    key = (name, band, target_is_a)
    if key not in _runs:
        _runs[key] = Run(ctx, name, band, target_is_a)
    return _runs[key]


def numbers(row):
    return (int(row["score"]), int(row["nm"]), int(row["b_start"]), int(row["b_end"]), int(row["a_start"]), int(row["a_end"]))


def failures_by_family(bad):
    out = {}
    for c, _msg in bad:
        out[c.family] = out.get(c.family, 0) + 1
    return out


BATCHES = ("designed", "with_n", "fuzz")
CONFIGS = [(band, tia, a) for band in (64, 256) for tia in (False, True) for a in (1, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("band,target_is_a,a", CONFIGS)
def test_all_six_numbers_equal_the_oracle(oracle, pkg, gpu_ctx, band, target_is_a, a):
    """ends_only = 0, the DP over the rows around the clusters (windows 1) and over all rows (0): score, NM and both spans are the oracle's for every pair"""
    for name in BATCHES:
        run = run_of(gpu_ctx, name, band, target_is_a)
        for windows in (1, 0):
            got, route, diag = run.audit(gpu_ctx, a, windows, 0)
            bad = []
            for k, c in enumerate(run.cases):
                if c.max_ed < 0:
                    assert route[k] == 3 and numbers(got[k]) == (0, 0, 0, 0, 0, 0)
                    continue
                exp = expected(oracle, name, run.idx[k], -int(diag[k]), band, a)
                if numbers(got[k]) != exp:
                    bad.append((c, (name, k, c.family, c.clean, c.place, int(route[k]), int(diag[k]), numbers(got[k]), exp)))
            print(name, "windows", windows, "routes 0/1/2/3:", [int((route == r).sum()) for r in range(4)], "wrong:", failures_by_family(bad))
            assert not bad, (len(bad), failures_by_family(bad), [m for _c, m in bad[:5]])


@pytest.mark.gpu
@pytest.mark.parametrize("band,target_is_a,a", CONFIGS)
def test_ends_only_extents_equal_the_oracle(oracle, pkg, gpu_ctx, band, target_is_a, a):
    """ends_only = 64 (K1's second stage): both spans are the oracle's, and the score is positive exactly where the oracle's is"""
    for name in BATCHES:
        run = run_of(gpu_ctx, name, band, target_is_a)
        got, route, diag = run.audit(gpu_ctx, a, 1, ENDS_KNOB)
        bad = []
        for k, c in enumerate(run.cases):
            if c.max_ed < 0:
                assert route[k] == 3 and numbers(got[k]) == (0, 0, 0, 0, 0, 0)
                continue
            exp = expected(oracle, name, run.idx[k], -int(diag[k]), band, a)
            have = numbers(got[k])
            if have[2:] != exp[2:] or (have[0] > 0) != (exp[0] > 0):
                bad.append((c, (name, k, c.family, c.clean, c.place, int(route[k]), int(diag[k]), have, exp)))
        print(name, "ends_only routes 0/1/2/3:", [int((route == r).sum()) for r in range(4)], "wrong:", failures_by_family(bad))
        assert not bad, (len(bad), failures_by_family(bad), [m for _c, m in bad[:5]])


@pytest.mark.gpu
@pytest.mark.parametrize("band,target_is_a", [(64, False), (64, True), (256, False), (256, True)])
def test_every_designed_family_takes_the_route_it_was_built_for(pkg, gpu_ctx, band, target_is_a):
    """closed form for lone edits at 16 bases or more, the rows around the clusters for clusters mid-sequence, all rows for an N, for stretches that do not fit the
    band and (ends_only) for a head and a tail that meet, none for a pair without a mapping -- as the audit reports it"""
    pinned, end_stretches = {}, set()
    for name in ("designed", "with_n"):
        run = run_of(gpu_ctx, name, band, target_is_a)
        for windows, ends_only, a in ((1, 0, 1), (0, 0, 1), (1, ENDS_KNOB, 1), (1, ENDS_KNOB, 5)):          # (a = 5: the score an end must keep is 72, not 8)
            _got, route, _diag = run.audit(gpu_ctx, a, windows, ends_only)
            for k, c in enumerate(run.cases):
                want = rc.expected_route(c, band, windows, ends_only, a)
                if want is not None:
                    assert route[k] == want, (name, k, c.family, c.clean, c.place, windows, ends_only, a, int(route[k]), want, len(c.target), len(c.query))
                    pinned.setdefault(c.family, set()).add(want)
                    if ends_only and want == 1 and c.family == "cluster behind a clean end":
                        end_stretches.add(c.place)
    assert {"lone", "two edits", "cluster mid-sequence", "cluster behind a clean end", "cluster at the head", "overhang", "score boundary", "long gap", "two clusters",
            "18 clusters", "does not fit", "head and tail meet", "no mapping"} <= set(pinned)
    assert all(f in pinned for f in ("N in the query", "N in the target", "N in both"))
    # ends_only's own route -- the DP over the stretch of an end, the closed form behind it -- is taken at the head, at the tail and at both; and so is the closed form
    assert end_stretches == {"head", "tail", "both"} and pinned["cluster behind a clean end"] == {0, 1, 2}

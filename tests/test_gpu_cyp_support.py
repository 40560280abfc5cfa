"""sp_cyp_consensus_support(_cohort): the support of the consensus regions of a CYP2D6 call by the reads of multi_mapping_details, on the simulated samples of
tests/cyp_fixture.py (120 reads: the count at which tests/test_gpu_cyp_pipeline.py calls these scenarios correctly), held to the composition written out here:
mappings -> segments -> sp_anchor_batch -> sp_affine_align_batch on 64 diagonals -> tests/pileup_ref.py -> sp_support_summarize.

Scenarios: *1/*4 (two copies) and *4x2/*1 (a duplication) of cyp_fixture, and *4+*68/*1 of tests/cyp_cases_real.py on the real database (several consensuses per
haplotype, a hybrid) at the 2,000 reads at which tests/test_gpu_cyp_real.py calls it correctly.  That sample's thousands of members are held to the same composition
with sp_pileup_batch in the place of pileup_ref.py (which is a Python loop per base: half a minute there); sp_pileup_batch is held to pileup_ref.py by its own tests
and, through the two small scenarios, here.

The designed sample plants one substitution in 60 % / 30 % of the members' segments of one consensus and hands the consensus and mappings from before the plant to
the step API: a consensus searched from the planted reads would follow the majority (DESIGN.md section 7.2 says the same of the HLA pass)."""
import numpy as np
import pytest

import pileup_ref as pr

pytestmark = pytest.mark.gpu

CONS_CAP = 32768


@pytest.fixture(scope="module")
def world(pkg, gpu_ctx):
    import cyp_fixture as cf
    import oracle_ffi as of
    from pb_starphase_amd import synth
    locus = synth.CypLocus(seed=11)
    db, d6 = cf.make_db(locus, synth, np.random.default_rng(5))
    cfg = of.default_cyp_config()
    templates = gpu_ctx.upload(db.seqs)
    problem = gpu_ctx.cyp_problem(templates, db.types, db.subtypes, db.deep, db.backbone, db.variants, db.is_vi, db.allele_subtypes, db.hap_matrix, cfg)
    out = {}
    for scenario in ("*1/*4", "*4x2/*1"):
        reads = cf.sample(locus, synth, np.random.default_rng(7), d6, scenario, 120)
        R = gpu_ctx.upload(reads)
        call, cons, mappings = pkg.database.cyp_problem_call_with_consensus(gpu_ctx, problem, R, CONS_CAP)
        assert call.status == 0 and call.n_consensus >= 2 and len(mappings) > 0
        out[scenario] = dict(reads=reads, R=R, call=call, cons=cons, mappings=mappings,
                             text=[pkg.database.cyp_consensus_of(cons, CONS_CAP, h) for h in range(call.n_consensus)])
    return dict(problem=problem, samples=out)


def expected(pkg, ctx, s, reads=None, device_pileup=False):
    """the composition, step by step: per consensus (table [length][8], summary dict)"""
    reads = reads or s["reads"]
    text = s["text"]
    live = [h for h in range(len(text)) if text[h]]
    members = [m for m in s["mappings"] if m.consensus in live]
    queries = [reads[m.read][m.read_start:m.read_end] for m in members]
    target = [live.index(m.consensus) for m in members]
    T, Q = ctx.upload([text[h] for h in live]), ctx.upload(queries)
    diag, votes = ctx.anchor_batch(T, Q, target, list(range(len(queries))))
    pairs = [(m, target[m], -int(diag[m]), 0 if votes[m] > 0 else -1) for m in range(len(queries))]
    aln, cigar, n_cigar = ctx.affine_align(Q, T, pairs, a=1, band=64, cigar_stride=4096)
    assert n_cigar.max() <= 4096
    if device_pileup:
        tabs = [pr.as_table(t) for t in ctx.pileup(Q, T, pairs, aln, cigar, n_cigar)]
    else:
        tabs = pr.pileup(queries, [len(text[h]) for h in live], pairs, aln, cigar, n_cigar)
    res = []
    for h in range(len(text)):
        if h not in live:
            res.append((np.zeros((0, 8), np.int64), pr.summary(np.zeros((0, 8), np.int64), 0, 0)))
            continue
        mine = [m for m in range(len(queries)) if target[m] == live.index(h)]
        res.append((tabs[live.index(h)], pr.summary(tabs[live.index(h)], len(mine), sum(int(aln[m]["score"]) > 0 for m in mine))))
    return res


@pytest.mark.parametrize("scenario", ["*1/*4", "*4x2/*1"])
def test_support_equals_the_composition(world, pkg, gpu_ctx, scenario):
    s = world["samples"][scenario]
    cols, sums = pkg.database.cyp_consensus_support(gpu_ctx, s["R"], s["call"], s["cons"], CONS_CAP, s["mappings"])
    want = expected(pkg, gpu_ctx, s)
    assert len(cols) == len(sums) == s["call"].n_consensus == len(want)
    for h, (tab_w, sm_w) in enumerate(want):
        tab = pr.as_table(cols[h])
        assert tab.shape == tab_w.shape and (tab == tab_w).all(), h
        assert sums[h] == sm_w, (h, sums[h], sm_w)
        assert (tab[:, 0] == tab[:, 1] + tab[:, 2:6].sum(axis=1) + tab[:, 6]).all()
        assert sums[h] == pkg.ffi.support_summarize(cols[h], sm_w["n_members"], sm_w["n_aligned"])
    assert sum(sm["n_members"] for sm in sums) == len(s["mappings"])                 # every record is a member of its consensus
    assert max(sm["median_depth"] for sm in sums) >= 3                               # the members do pile up under a consensus
    # without the table: the same summaries, computed on the device
    none, sums2 = pkg.database.cyp_consensus_support(gpu_ctx, s["R"], s["call"], s["cons"], CONS_CAP, s["mappings"], want_cols=False)
    assert none is None and sums2 == sums


def test_hybrid_sample_of_the_real_database(pkg, gpu_ctx):
    """*4+*68/*1: a CYP2D6::CYP2D7 hybrid beside two CYP2D6 copies"""
    import json
    import cyp_cases_real as cr
    from pb_starphase_amd import synth
    cfg, gene_def = cr.load_db()
    locus = synth.Chr22Locus(cfg, gene_def, seed=3)
    cdb = pkg.ffi.CypDb(gpu_ctx, cfg, gene_def, locus.sequence, locus.start)
    haps, truth = {n: (h, e) for n, h, e in cr.scenarios(locus)}["*4+*68/*1"]
    reads = locus.sample(np.random.default_rng(7), haps, 2000)
    R = gpu_ctx.upload(reads)
    call, cons, mappings = pkg.database.cyp_call_with_consensus(cdb, R, CONS_CAP)
    assert call.status == 0 and sorted([call.hap1.decode(), call.hap2.decode()]) == sorted(truth)
    text = [pkg.database.cyp_consensus_of(cons, CONS_CAP, h) for h in range(call.n_consensus)]
    s = dict(reads=reads, text=text, mappings=mappings)
    hybrids = [h for h in range(call.n_consensus) if call.cons_type[h] == 8]              # SP_CYP_HYBRID
    assert hybrids and call.n_consensus > 4 and len(mappings) > pkg.ffi.SP_PILEUP_WAVES
    cols, sums = pkg.database.cyp_consensus_support(gpu_ctx, R, call, cons, CONS_CAP, mappings)
    want = expected(pkg, gpu_ctx, s, device_pileup=True)
    for h, (tab_w, sm_w) in enumerate(want):
        tab = pr.as_table(cols[h])
        assert tab.shape == tab_w.shape and (tab == tab_w).all(), h
        assert sums[h] == sm_w, (h, sums[h], sm_w)
        assert (tab[:, 0] == tab[:, 1] + tab[:, 2:6].sum(axis=1) + tab[:, 6]).all()
    assert sum(sm["n_members"] for sm in sums) == len(mappings)
    assert all(sums[h]["n_aligned"] >= 3 and sums[h]["median_depth"] >= 3 for h in hybrids)
    got = json.loads(pkg.database.cyp_support_json(call, text, cols, sums))
    assert len(got) == call.n_consensus
    for h in hybrids:
        key = [k for k in got if k.startswith(f"{h}_")][0]
        assert got[key]["region_type"] == call.cons_subtype[h].value.decode() == key.split("_", 1)[1] and "CYP2D6::CYP2D7" in key


def test_cohort_of_two_samples_equals_each_sample_alone(world, pkg, gpu_ctx):
    a, b = world["samples"]["*1/*4"], world["samples"]["*4x2/*1"]
    both = pkg.database.cyp_consensus_support_cohort(gpu_ctx, [a["R"], b["R"]], [a["call"], b["call"]], [a["cons"], b["cons"]], CONS_CAP, [a["mappings"], b["mappings"]])
    for s, (cols, sums) in zip((a, b), both):
        cols1, sums1 = pkg.database.cyp_consensus_support(gpu_ctx, s["R"], s["call"], s["cons"], CONS_CAP, s["mappings"])
        assert sums == sums1 and [c.tobytes() for c in cols] == [c.tobytes() for c in cols1]


@pytest.mark.parametrize("fraction,contested", [(0.6, True), (0.3, False)])
def test_designed_sample(world, pkg, gpu_ctx, fraction, contested):
    s = world["samples"]["*1/*4"]
    cols0, sums0 = pkg.database.cyp_consensus_support(gpu_ctx, s["R"], s["call"], s["cons"], CONS_CAP, s["mappings"])
    clean = [x for x in range(len(sums0)) if sums0[x]["n_contested"] == 0 and sums0[x]["n_aligned"] >= 10]     # nothing contested before the plant
    assert clean, [(sm["n_aligned"], sm["n_contested"]) for sm in sums0]
    h = max(clean, key=lambda x: sums0[x]["n_aligned"])
    before = list(pkg.ffi.support_contested(cols0[h]))
    assert before == []
    # a column every aligned member spans with '=', and where in each member's segment it lies: from the composition's alignments
    text = s["text"]
    members = [m for m in s["mappings"] if m.consensus == h]
    queries = [s["reads"][m.read][m.read_start:m.read_end] for m in members]
    T, Q = gpu_ctx.upload([text[h]]), gpu_ctx.upload(queries)
    diag, votes = gpu_ctx.anchor_batch(T, Q, [0] * len(queries), list(range(len(queries))))
    pairs = [(m, 0, -int(diag[m]), 0 if votes[m] > 0 else -1) for m in range(len(queries))]
    aln, cigar, n_cigar = gpu_ctx.affine_align(Q, T, pairs, a=1, band=64, cigar_stride=4096)
    # the column: one that every spanning member covers inside a run of '=' with 10 matching bases on either side, so that the planted base stays a lone mismatch
    # (next to an indel of the read the aligner may spell a substitution another way)
    runs, roomy = [], np.zeros(len(text[h]), np.int64)
    for m in range(len(queries)):
        j, q = int(aln[m]["b_start"]), int(aln[m]["a_start"])
        for k in range(int(n_cigar[m])):
            op, n = int(cigar[m][k]) & 15, int(cigar[m][k]) >> 4
            if op == 7:
                runs.append((m, j, n, q))
                roomy[j + 10:max(j + 10, j + n - 10)] += 1
            j += n if op != 1 else 0
            q += n if op != 2 else 0
    good = np.flatnonzero((roomy == cols0[h]["depth"]) & (cols0[h]["depth"] >= 10) & (cols0[h]["ins"] == 0))
    assert len(good) > 0
    col = int(good[np.argmax(cols0[h]["depth"][good])])
    assert cols0[h]["eq"][col] == cols0[h]["depth"][col]
    at = {m: q + (col - j) for m, j, n, q in runs if j <= col < j + n}
    spanning = sorted(at)
    assert len(spanning) == int(cols0[h]["depth"][col])
    planted = spanning[:int(round(fraction * len(spanning)))]
    new_base = "ACGT"[("ACGT".index(text[h][col]) + 1) % 4]
    reads = list(s["reads"])
    for m in planted:
        r, p = members[m].read, members[m].read_start + at[m]
        assert reads[r][p] == text[h][col]
        reads[r] = reads[r][:p] + new_base + reads[r][p + 1:]
    R2 = gpu_ctx.upload(reads)
    cols, sums = pkg.database.cyp_consensus_support(gpu_ctx, R2, s["call"], s["cons"], CONS_CAP, s["mappings"])
    where = list(pkg.ffi.support_contested(cols[h]))
    assert int(cols[h]["x"][col]["ACGT".index(new_base)]) == len(planted)
    assert col not in before and where == sorted(before + ([col] if contested else [])) and sums[h]["n_contested"] == len(where)
    assert 2 * len(planted) >= len(spanning) if contested else 2 * len(planted) < len(spanning)
    want = expected(pkg, gpu_ctx, s, reads)
    assert (pr.as_table(cols[h]) == want[h][0]).all() and sums[h] == want[h][1]


def test_a_failed_call_gives_zeroed_summaries(world, pkg, gpu_ctx):
    import ctypes as C
    ffi = pkg.ffi
    R = gpu_ctx.upload(["ACGT" * 500])
    call, cons, mappings = pkg.database.cyp_problem_call_with_consensus(gpu_ctx, world["problem"], R, CONS_CAP)
    assert call.status == 1 and mappings == []
    off = np.full(ffi.SP_CYP_MAXCONS + 1, 7, np.uint64)
    sm = np.full(ffi.SP_CYP_MAXCONS, 0xFF, ffi.SUPPORT_DTYPE)
    bad = world["samples"]["*1/*4"]["call"]
    failed = ffi.sp_cyp_call()
    C.memmove(C.byref(failed), C.byref(bad), C.sizeof(ffi.sp_cyp_call))
    failed.status = 7                                                                # a call that failed after its consensuses were made
    for c in (call, failed):
        rc = pkg.database._lib().sp_cyp_consensus_support(gpu_ctx._h, R._h, C.byref(c), C.cast(cons, C.c_void_p), CONS_CAP, None, 0, ffi._ptr(off), None, 0, ffi._ptr(sm))
        H = max(0, c.n_consensus)
        assert rc == ffi.SP_OK and not off[:H + 1].any() and not sm[:H].tobytes().strip(b"\0")
        assert pkg.database.cyp_support_json(c, [""] * H, [np.zeros(0, ffi.PILEUP_DTYPE)] * H, [{}] * H) == "{}"

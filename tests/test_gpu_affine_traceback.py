"""sp_affine_align_batch / sp_hla_realign_cigars: HOW a pair aligns under the reference's scores -- the traceback of the two-piece affine DP (sp_affine.hip).
  1. bit-exact against the Python statement (tests/affine_traceback_ref.py: oracle/affine.c with back pointers) on small fuzzed pairs
  2. exact invariants on every accepted read of the 10,000-read configs[1] workload: spans, NM, column types and the affine score of the path are the record's
  3. against the minimap2 restatement (oracle/mm2.c) on the first 300 accepted reads: same NM, spans and score on all of them, the share of byte-identical
     CIGARs measured and gated from below
  4. overflow, empty batches, skipped pairs"""
import numpy as np
import pytest

import affine_traceback_ref as ar
import oracle_ffi as of

pytestmark = pytest.mark.gpu

OPNUM = {"=": 7, "X": 8, "I": 1, "D": 2}
# Share of the 300 reads whose CIGAR is byte for byte the minimap2 restatement's.  Co-optimal alignments may place a gap elsewhere (minimap2 aligns piecewise between its
# seeds; this DP takes the forward pass's own ties), so the share is measured, not argued: 286 / 300 = 0.953 on the MI355X for this sample; NM, spans and score are equal on all 300.
MM2_SAME_CIGAR_MIN = 0.95


def test_bit_exact_on_small_pairs(oracle, pkg, gpu_ctx):
    rng = np.random.default_rng(20)
    pairs = ar.fuzz_pairs(rng, 200)
    targets, queries = [p[0] for p in pairs], [p[1] for p in pairs]
    T, Q = gpu_ctx.upload(targets), gpu_ctx.upload(queries)
    seen = dict(long_gap=0, ambi=0, zero=0, x=0, i=0, d=0, wide=0, a5=0)
    config = lambda x: (256 if x % 4 == 3 else 64, 5 if x % 3 == 2 else 1)                    # every pair under one band and one score set, all four combinations met
    for band, a in ((64, 1), (64, 5), (256, 1), (256, 5)):
        idx = [x for x in range(200) if config(x) == (band, a)]
        rows = [(x, x, pairs[x][2]) for x in idx]
        out, cigar, n_cigar = gpu_ctx.affine_align(Q, T, rows, a=a, band=band, cigar_stride=512)
        plain = gpu_ctx.affine_rescore(Q, T, rows, a=a, band=band)
        assert out.tobytes() == plain.tobytes(), (band, a)                                   # the record sp_affine_rescore_batch writes for the same call
        for k, x in enumerate(idx):
            t, q, d = pairs[x]
            exp = of.oracle_affine(oracle, t, q, -d, band, a)
            have = tuple(int(out[k][f]) for f in ("score", "nm", "b_start", "b_end", "a_start", "a_end"))
            assert have == tuple(exp), (x, band, a, have, exp)
            ref_out, ref_ops = ar.affine_traceback(t, q, -d, band, a=a)
            assert tuple(ref_out) == have
            ops = ar.decode_ops(cigar[k], int(n_cigar[k]))
            assert ops == ref_ops, (x, band, a, d, ops, ref_ops)
            if have[0] == 0:
                assert n_cigar[k] == 0
                seen["zero"] += 1
                continue
            nm, score = ar.check_ops(ops, t, q, have[2], have[3], have[4], have[5], a=a)
            assert (nm, score) == (have[1], have[0])
            seen["long_gap"] += any(n > 20 and op in (1, 2) for n, op in ops)
            seen["ambi"] += "N" in t[have[2]:have[3]] or "N" in q[have[4]:have[5]]
            seen["wide"] += band == 256
            seen["a5"] += a == 5
            for key, op in (("x", 8), ("i", 1), ("d", 2)):
                seen[key] += any(o == op for _, o in ops)
    assert all(v >= 5 for v in seen.values()), seen            # every class of the fuzz was met


@pytest.fixture(scope="module")
def workload(pkg, gpu_ctx):
    from pb_starphase_amd import synth
    fx = synth.HlaFixture()
    db = fx.make_db(pkg, gpu_ctx)
    wl = synth.Config2Workload(fx, n_reads=10000, seed=1000)
    R = gpu_ctx.upload(wl.reads)
    rec = db.realign_reads(R)
    gpu_ctx.profile_reset()
    cigar, n_cigar = db.realign_cigars(R, rec, cigar_stride=1024)
    print("sp_hla_realign_cigars, 10,000 reads: affine_align kernels (ms, launches, pairs)", gpu_ctx.profile_get("affine_align"))
    return fx, wl, rec, cigar, n_cigar


def test_every_accepted_read_of_the_workload(workload):
    fx, wl, rec, cigar, n_cigar = workload
    ok = np.flatnonzero(rec["status"] == 0)
    assert len(ok) > 9000 and (n_cigar[rec["status"] != 0] == 0).all()
    assert n_cigar.max() <= cigar.shape[1]
    for r in ok:
        q = rec[r]
        ops = ar.decode_ops(cigar[r], int(n_cigar[r]))
        nm, score = ar.check_ops(ops, fx.dna_fwd(int(q["best_allele"])), wl.reads[r], int(q["mm2_t_start"]), int(q["mm2_t_end"]), int(q["mm2_q_start"]), int(q["mm2_q_end"]))
        assert nm == q["mm2_nm"] and score == q["mm2_score"], (r, nm, score, q["mm2_nm"], q["mm2_score"])


def test_against_the_minimap2_restatement(oracle, workload):
    import mm2_ffi
    fx, wl, rec, cigar, n_cigar = workload
    mm = mm2_ffi.Mm2(oracle)
    # the first 300 accepted reads in QNAME order, none left out: the workload's reads have no names of their own, read r is "read/<r>" and the order is that of the strings
    sample = sorted(np.flatnonzero(rec["status"] == 0).tolist(), key=lambda r: f"read/{r}")[:300]
    assert len(sample) == 300
    same = 0
    for r in sample:
        q = rec[r]
        target, read = fx.dna_fwd(int(q["best_allele"])), wl.reads[r]
        hits = [h for h in mm.map_pair(target, read) if not h["rev"] and h["primary"]]
        assert hits, r
        h = hits[0]
        theirs = []
        for n, op in h["cigar"]:                                # (runs of one op next to one another are one run)
            if theirs and theirs[-1][1] == OPNUM[op]:
                theirs[-1] = (theirs[-1][0] + n, OPNUM[op])
            else:
                theirs.append((n, OPNUM[op]))
        nm, score = ar.check_ops(theirs, target, read, h["t_start"], h["t_end"], h["q_start"], h["q_end"])
        assert (h["t_start"], h["t_end"], h["q_start"], h["q_end"]) == (q["mm2_t_start"], q["mm2_t_end"], q["mm2_q_start"], q["mm2_q_end"]), r
        assert nm == h["nm"] == q["mm2_nm"] and score == q["mm2_score"], (r, nm, h["nm"], q["mm2_nm"], score, q["mm2_score"])
        same += theirs == ar.decode_ops(cigar[r], int(n_cigar[r]))
    print(f"byte-identical CIGARs: {same} / 300")
    assert same >= MM2_SAME_CIGAR_MIN * 300


def test_overflow_and_empties(pkg, gpu_ctx):
    rng = np.random.default_rng(21)
    pairs = ar.fuzz_pairs(rng, 16)
    T, Q = gpu_ctx.upload([p[0] for p in pairs]), gpu_ctx.upload([p[1] for p in pairs])
    rows = [(x, x, pairs[x][2]) for x in range(16)]
    out, cigar, n_cigar = gpu_ctx.affine_align(Q, T, rows, cigar_stride=256)
    assert n_cigar.max() >= 4
    out2, small, n2 = gpu_ctx.affine_align(Q, T, rows, cigar_stride=2)
    assert out2.tobytes() == out.tobytes() and (n2 == n_cigar).all()                          # SP_OK, the true counts ...
    for x in range(16):
        k = min(2, int(n_cigar[x]))
        assert (small[x, :k] == cigar[x, :k]).all()                                           # ... and a prefix
    out3, _c, n3 = gpu_ctx.affine_align(Q, T, rows, cigar_stride=0)
    assert out3.tobytes() == out.tobytes() and (n3 == n_cigar).all()
    out0, c0, n0 = gpu_ctx.affine_align(Q, T, [])
    assert len(out0) == 0 and len(n0) == 0
    skipped = [(x, x, pairs[x][2], -1 if x % 2 else 0) for x in range(16)]                     # max_ed < 0: the callers' "skip"
    out4, c4, n4 = gpu_ctx.affine_align(Q, T, skipped, cigar_stride=256)
    for x in range(16):
        if x % 2:
            assert out4[x]["score"] == 0 and n4[x] == 0
        else:
            assert out4[x] == out[x] and n4[x] == n_cigar[x] and (c4[x, :n4[x]] == cigar[x, :n4[x]]).all()


def test_reads_across_a_long_gap_take_the_wide_band(pkg, gpu_ctx):
    """sp_hla_realign_cigars derives the band from the record's cell: a read with 60 bases more or fewer than its allele in the middle has a cell whose ends lie more than
    32 diagonals apart, was re-scored on 256 diagonals, and its CIGAR -- with the gap in one piece -- reproduces the record"""
    from pb_starphase_amd import synth
    fx = synth.HlaFixture()
    db = fx.make_db(pkg, gpu_ctx)
    wl = synth.Config2Workload(fx, n_reads=120, seed=77)
    rng = np.random.default_rng(78)
    reads = []
    for r, read in enumerate(wl.reads):
        al = fx.dna_fwd(wl.read_truth[r][1])
        p = read.find(al[len(al) // 2:len(al) // 2 + 40])
        if p < 0:
            continue
        reads.append(read[:p] + "".join(rng.choice(list("ACGT"), 60)) + read[p:] if len(reads) % 2 else read[:p] + read[p + 60:])
    assert len(reads) >= 60
    R = gpu_ctx.upload(reads)
    rec = db.realign_reads(R)
    cigar, n_cigar = db.realign_cigars(R, rec, cigar_stride=1024)
    shift = (rec["aln"]["b_end"] - rec["aln"]["a_end"]) - (rec["aln"]["b_start"] - rec["aln"]["a_start"])
    wide = np.flatnonzero((rec["status"] == 0) & (np.abs(shift) > 32))
    print("reads with the gap:", len(reads), "accepted across it:", len(wide))
    assert len(wide) >= 20
    for r in wide:
        q = rec[r]
        ops = ar.decode_ops(cigar[r], int(n_cigar[r]))
        nm, score = ar.check_ops(ops, fx.dna_fwd(int(q["best_allele"])), reads[r], int(q["mm2_t_start"]), int(q["mm2_t_end"]), int(q["mm2_q_start"]), int(q["mm2_q_end"]))
        assert nm == q["mm2_nm"] and score == q["mm2_score"], (r, nm, score, q["mm2_nm"], q["mm2_score"])
        assert any(n >= 55 and op in (1, 2) for n, op in ops), (r, ops)

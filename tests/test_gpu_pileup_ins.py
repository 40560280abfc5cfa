"""sp_pileup_ins_batch and sp_align_pileup_ins_batch (sp_pileup.hip): the inserted strings behind every column, held record for record to tests/pileup_ins_ref.py
over the op rows of sp_affine_align_batch.  The main batch runs on 256 diagonals (a run of 32 bases or more leaves the 64-diagonal band); the retry batch and the
sliced batch on 64 diagonals, and on 256 for the pairs that found nothing there: the rule of retry_band.

The main batch plants, on targets of 300 to 5,000 bases: runs of 1, 2, 31, 32, 33, 64, 65 and 100 bases; a run behind the last column of a tile and behind the first
of the next; two strings of one length and one count on one column; two strings of 70 bases that share their first 64; one string carried by 200 members; 40 distinct
strings on one column; an insertion that holds an N; a target no pair names.  The retry batch holds a member that aligns on the 256-diagonal retry only.  Hand-made op rows put a run behind
column 0 and behind the last aligned column of a member that ends inside the target (the aligner clips both).  A batch of SP_ALIGN_PILEUP_SLICE + 1 members of 120
bases crosses the slice and puts more than SP_PILEUP_INS_LDS_RUNS runs on one tile (the sort outside LDS)."""
import numpy as np
import pytest

import pileup_ins_ref as ref

pytestmark = pytest.mark.gpu

KW = dict(band=256, retry_band=0)                                                                      # the main batch's band

BASES = "ACGT"
LENGTHS = (1, 2, 31, 32, 33, 64, 65, 100)


def rand_seq(rng, n):
    return "".join(BASES[i] for i in rng.integers(0, 4, n))


def foreign(target, c):
    """the bases that are neither target[c] nor target[c + 1]: a string over them, planted behind column c, can sit nowhere else"""
    return [b for b in BASES if b not in (target[c], target[c + 1])]


def planted(rng, target, c, n):
    """n bases to plant behind column c: random, the ends foreign to the flanks"""
    f = foreign(target, c)
    s = list(rand_seq(rng, n))
    s[0], s[-1] = f[0], f[-1]
    return "".join(s)


def member(target, c, s, flank=150):
    """(query, first target column): target[c - flank + 1 .. c] + s + target[c + 1 .. c + flank]"""
    lo, hi = max(0, c + 1 - flank), min(len(target), c + 1 + flank)
    return target[lo:c + 1] + s + target[c + 1:hi], lo


def rows_by_rule(ctx, A, B, pairs, stride):
    """sp_affine_align_batch on 64 diagonals, and on 256 for the attempted pairs that came back with score 0 or without ops"""
    aln, cigar, n_cigar = ctx.affine_align(A, B, pairs, a=1, band=64, cigar_stride=stride)
    again = [i for i, p in enumerate(pairs) if p[3] >= 0 and (int(aln[i]["score"]) <= 0 or int(n_cigar[i]) == 0)]
    if again:
        aln2, cigar2, n2 = ctx.affine_align(A, B, [pairs[i] for i in again], a=1, band=256, cigar_stride=stride)
        for k, i in enumerate(again):
            aln[i], cigar[i], n_cigar[i] = aln2[k], cigar2[k], n2[k]
    assert int(n_cigar.max()) <= stride
    return aln, cigar, n_cigar, again


def col_offsets(B):
    off = np.zeros(B.n + 1, np.uint64)
    off[1:] = np.cumsum([int(x) for x in B.lengths])
    return off


def check_against_cols(rows, cols, off):
    """count + n_other over a column's records is the column's ins, and no other column has one"""
    want = {int(off[t]) + j: int(c["ins"]) for t, tab in enumerate(cols) for j, c in enumerate(tab) if int(c["ins"])}
    assert ref.ins_per_column(rows) == want


@pytest.fixture(scope="module")
def batch(pkg, gpu_ctx):
    ffi = pkg.ffi
    T = ffi.SP_PILEUP_TILE
    rng = np.random.default_rng(77)
    targets = [rand_seq(rng, 300), rand_seq(rng, 5000), rand_seq(rng, 400), rand_seq(rng, 600)]        # target 2 gets no pair
    queries, pairs, plan = [], [], {}

    def add(t, c, s, shift=0, tag=None, flank=150):
        q, lo = member(targets[t], c, s, flank)
        queries.append(q)
        pairs.append((len(queries) - 1, t, lo + shift, 0))
        if tag:
            plan.setdefault(tag, []).append((t, c, s))

    t1 = targets[1]
    for k, n in enumerate(LENGTHS):                                                                    # every length, each on a column of its own
        add(1, 300 + 400 * k, planted(rng, t1, 300 + 400 * k, n), tag="len")
    for c in (T - 1, T):                                                                               # behind a tile's last column, behind the next one's first
        add(1, c, foreign(t1, c)[0] * 3, tag="edge")
    x, y = foreign(t1, 4200)[0], foreign(t1, 4200)[-1]
    assert x != y
    for s in (x + y + x, y + x + y, x + y + x, y + x + y):                                             # a tie: one length, one count, two strings
        add(1, 4200, s, tag="tie")
    head = planted(rng, t1, 4500, 64)
    for tail in (foreign(t1, 4500)[0] * 6, foreign(t1, 4500)[-1] * 6):                                 # 70 bases each, the first 64 shared
        add(1, 4500, head + tail, tag="long")
    t3 = targets[3]
    for _ in range(200):                                                                               # one string, 200 members
        add(3, 150, foreign(t3, 150)[0] * 2, tag="many")
    f = foreign(t3, 400)
    for k in range(40):                                                                                # 40 distinct strings of 6 bases on one column
        add(3, 400, "".join(f[(k >> b) & 1] for b in range(6)), tag="forty")
    add(1, 3700, foreign(t1, 3700)[0] + "N" + foreign(t1, 3700)[0], tag="n")                           # an insertion that holds an N
    add(1, 3700, foreign(t1, 3700)[0] * 3)                                                             # ... and a listed one on the same column
    add(0, 150, foreign(targets[0], 150)[0] * 4)
    A, B = gpu_ctx.upload(queries), gpu_ctx.upload(targets)
    aln, cigar, n_cigar = gpu_ctx.affine_align(A, B, pairs, a=1, band=256, cigar_stride=256)
    assert int(n_cigar.max()) <= 256
    off = col_offsets(B)
    want = ref.records(pairs, aln, cigar, n_cigar, queries, off)
    got = gpu_ctx.align_pileup(A, B, pairs, insertions=True, **KW)
    return dict(ffi=ffi, T=T, targets=targets, queries=queries, pairs=pairs, plan=plan, A=A, B=B, aln=aln, cigar=cigar, n_cigar=n_cigar, off=off, want=want, got=got)


def test_the_batch_holds_the_designed_cases(batch):
    b, T, off = batch, batch["T"], batch["off"]
    want = b["want"]
    assert {r[1] for r in want} >= set(LENGTHS) | {70}
    cols = {r[0] for r in want}
    assert int(off[1]) + T - 1 in cols and int(off[1]) + T in cols
    tie = [r for r in want if r[0] == int(off[1]) + 4200]
    assert len(tie) == 2 and tie[0][2] == tie[1][2] == 2 and tie[0][1] == tie[1][1] == 3 and tie[0][3] < tie[1][3]
    long = [r for r in want if r[1] == 70]
    assert len(long) == 2 and long[0][3:5] == long[1][3:5] and long[0][5] != long[1][5] and long[0][0] == long[1][0]
    assert any(r[2] == 200 for r in want)
    assert len([r for r in want if r[0] == int(off[3]) + 400]) == 40
    assert [r[8] for r in want if r[0] == int(off[1]) + 3700] == [1]                                   # the N run counts in n_other of its column's one record
    assert any(r[0] < int(off[1]) for r in want)
    assert not any(int(off[2]) <= r[0] < int(off[3]) for r in want)


def test_the_host_rows_call_equals_the_reference(batch, gpu_ctx):
    b = batch
    got = gpu_ctx.pileup_ins(b["A"], b["B"], b["pairs"], b["aln"], b["cigar"], b["n_cigar"])
    assert ref.as_rows(got) == b["want"]
    check_against_cols(ref.as_rows(got), gpu_ctx.pileup(b["A"], b["B"], b["pairs"], b["aln"], b["cigar"], b["n_cigar"]), b["off"])


def test_the_device_resident_call_equals_the_reference(batch):
    b = batch
    aln, cols, sums, ins = b["got"]
    assert aln.tobytes() == b["aln"].tobytes()
    assert ref.as_rows(ins) == b["want"]
    check_against_cols(ref.as_rows(ins), cols, b["off"])


def test_the_strings_come_back(batch, pkg):
    b = batch
    aln, cols, sums, ins = b["got"]
    for r in ins:
        if int(r["len"]) == 0:
            continue
        q = b["pairs"][int(r["first_pair"])][0]
        s = pkg.ffi.support_ins_string(r, b["A"], q)
        assert s == b["queries"][q][int(r["first_qpos"]):int(r["first_qpos"]) + int(r["len"])]
        assert ref.key_of(s) == (int(r["len"]), int(r["p0"]), int(r["p1"]), int(r["h"]))


def test_without_a_list_the_call_is_the_band_call(batch, gpu_ctx):
    b = batch
    old = gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"], **KW)
    aln, cols, sums, ins = b["got"]
    assert old[0].tobytes() == aln.tobytes() and old[2] == sums
    assert all(o.tobytes() == c.tobytes() for o, c in zip(old[1], cols))
    ffi, lib = b["ffi"], b["ffi"].lib()
    import ctypes as C
    rows = np.zeros(len(b["pairs"]), ffi.PAIR_DTYPE)
    for i, pr in enumerate(b["pairs"]):
        rows[i] = pr
    out = np.zeros(len(rows), ffi.AFFINE_DTYPE)
    table = np.zeros(int(b["off"][-1]), ffi.PILEUP_DTYPE)
    sm = np.zeros(b["B"].n, ffi.SUPPORT_DTYPE)
    op = ffi.sp_affine_opts(1, 4, 6, 2, 26, 1, 1)
    launches = gpu_ctx.profile_get("pileup_ins_collect")[1]
    rc = lib.sp_align_pileup_ins_batch(gpu_ctx._h, b["A"]._h, b["B"]._h, ffi._ptr(rows), len(rows), C.byref(op), 256, 0, ffi._ptr(b["off"]), ffi._ptr(out), ffi._ptr(table),
                                       ffi._ptr(sm), None, None, None, 0, None)                        # ins = NULL: the old pass
    assert rc == ffi.SP_OK and gpu_ctx.profile_get("pileup_ins_collect")[1] == launches
    assert out.tobytes() == aln.tobytes() and table.tobytes() == np.concatenate(cols).tobytes()


def test_a_warm_call_allocates_nothing(batch, gpu_ctx):
    b = batch
    before = gpu_ctx.profile_get("pool:device")
    again = gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"], insertions=True, **KW)
    assert gpu_ctx.profile_get("pool:device")[1:] == before[1:]
    assert again[3].tobytes() == b["got"][3].tobytes()
    before = gpu_ctx.profile_get("pool:device")
    gpu_ctx.pileup_ins(b["A"], b["B"], b["pairs"], b["aln"], b["cigar"], b["n_cigar"])
    gpu_ctx.pileup_ins(b["A"], b["B"], b["pairs"], b["aln"], b["cigar"], b["n_cigar"])
    warm = gpu_ctx.profile_get("pool:device")
    gpu_ctx.pileup_ins(b["A"], b["B"], b["pairs"], b["aln"], b["cigar"], b["n_cigar"])
    assert gpu_ctx.profile_get("pool:device")[1:] == warm[1:]


def test_a_list_one_record_short_is_asked_for_again(batch, gpu_ctx):
    b, ffi = batch, batch["ffi"]
    n = len(b["want"])
    rc, ins, n_ins = gpu_ctx.pileup_ins(b["A"], b["B"], b["pairs"], b["aln"], b["cigar"], b["n_cigar"], ins_cap=n - 1)
    assert rc == ffi.SP_ERR_CAPACITY and n_ins == n and ins is None
    rc, ins, n_ins = gpu_ctx.pileup_ins(b["A"], b["B"], b["pairs"], b["aln"], b["cigar"], b["n_cigar"], ins_cap=n)
    assert rc == ffi.SP_OK and ref.as_rows(ins) == b["want"]
    res = gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"], insertions=True, ins_cap=n - 1, **KW)
    assert res[3] == (ffi.SP_ERR_CAPACITY, None, n)
    assert res[0].tobytes() == b["aln"].tobytes()                                                      # everything else is complete
    res = gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"], insertions=True, ins_cap=n, **KW)
    assert res[3][0] == ffi.SP_OK and ref.as_rows(res[3][1]) == b["want"]


def test_a_member_that_aligns_on_the_retry_alone_carries_its_insertion(pkg, gpu_ctx):
    rng = np.random.default_rng(9)
    target = rand_seq(rng, 300)
    queries, pairs = [], []
    for c, shift, flank in ((100, 0, 150), (180, 0, 150), (264, 104, 35)):
        # the last one: 73 bases at the target's end on a diagonal 104 off -- the 64-diagonal rectangle is empty, the 256-diagonal one holds the member
        q, lo = member(target, c, foreign(target, c)[0] * 3, flank)
        queries.append(q)
        pairs.append((len(queries) - 1, 0, lo + shift, 0))
    A, B = gpu_ctx.upload(queries), gpu_ctx.upload([target])
    aln, cigar, n_cigar, again = rows_by_rule(gpu_ctx, A, B, pairs, 64)
    assert again == [2] and int(aln[2]["score"]) > 0
    want = ref.records(pairs, aln, cigar, n_cigar, queries, [0, 300])
    assert [(r[0], r[1], r[6]) for r in want] == [(100, 3, 0), (180, 3, 1), (264, 3, 2)]
    got = gpu_ctx.align_pileup(A, B, pairs, band=64, retry_band=256, insertions=True, band_used=True)
    assert list(got[3]) == [64, 64, 256] and ref.as_rows(got[4]) == want
    check_against_cols(ref.as_rows(got[4]), got[1], [0, 300])


def test_hand_made_rows_behind_column_0_and_behind_a_members_last_column(pkg, gpu_ctx):
    ffi = pkg.ffi
    rng = np.random.default_rng(5)
    target = rand_seq(rng, 300)
    queries = [target[0] + "GAT" + target[1:200], target[50:150] + "CC", target[0] + "GAT" + target[1:100]]
    pairs = [(0, 0, 0, 0), (1, 0, 50, 0), (2, 0, 0, 0)]
    aln = np.zeros(3, ffi.AFFINE_DTYPE)
    aln[0] = (1, 0, 0, 203, 0, 200)
    aln[1] = (1, 0, 0, 102, 50, 150)
    aln[2] = (1, 0, 0, 103, 0, 100)
    cigar = np.zeros((3, 4), np.uint32)
    cigar[0, :3] = [(1 << 4) | 7, (3 << 4) | 1, (199 << 4) | 7]
    cigar[1, :2] = [(100 << 4) | 7, (2 << 4) | 1]
    cigar[2, :3] = [(1 << 4) | 7, (3 << 4) | 1, (99 << 4) | 7]
    n_cigar = np.array([3, 2, 3], np.uint32)
    A, B = gpu_ctx.upload(queries), gpu_ctx.upload([target])
    got = ref.as_rows(gpu_ctx.pileup_ins(A, B, pairs, aln, cigar, n_cigar))
    assert got == ref.records(pairs, aln, cigar, n_cigar, queries, [0, 300])
    assert [(r[0], r[1], r[2], r[6], r[7]) for r in got] == [(0, 3, 2, 0, 1), (149, 2, 1, 1, 100)]
    check_against_cols(got, gpu_ctx.pileup(A, B, pairs, aln, cigar, n_cigar), [0, 300])


def test_a_batch_without_an_insertion_has_an_empty_list(pkg, gpu_ctx):
    rng = np.random.default_rng(6)
    targets = [rand_seq(rng, 700), rand_seq(rng, 300)]
    queries = [targets[0][100:400], targets[0][300:650]]
    pairs = [(0, 0, 100, 0), (1, 0, 300, 0)]
    A, B = gpu_ctx.upload(queries), gpu_ctx.upload(targets)
    aln, cols, sums, ins = gpu_ctx.align_pileup(A, B, pairs, insertions=True)
    assert len(ins) == 0 and int(aln["score"].min()) > 0
    aln, cigar, n_cigar = gpu_ctx.affine_align(A, B, pairs, a=1, band=64, cigar_stride=64)
    assert len(gpu_ctx.pileup_ins(A, B, pairs, aln, cigar, n_cigar)) == 0
    rc, ins, n_ins = gpu_ctx.pileup_ins(A, B, pairs, aln, cigar, n_cigar, ins_cap=0)
    assert rc == pkg.ffi.SP_OK and n_ins == 0


def test_more_pairs_than_a_slice_and_more_runs_than_lds_holds(pkg, gpu_ctx):
    ffi = pkg.ffi
    n = ffi.SP_ALIGN_PILEUP_SLICE + 1
    rng = np.random.default_rng(8)
    target = rand_seq(rng, 300)
    spots = [60, 110, 160, 210]
    strings = {c: [foreign(target, c)[0] * k for k in (1, 2, 3)] for c in spots}
    queries, pairs = [], []
    for i in range(n):
        c = spots[i % 4]
        s = strings[c][(i // 4) % 3]
        q = target[c - 59:c + 1] + s + target[c + 1:c + 61 - len(s)]
        assert len(q) == 120
        queries.append(q)
        pairs.append((i, 0, c - 59, 0))
    A, B = gpu_ctx.upload(queries), gpu_ctx.upload([target])
    aln, cigar, n_cigar, again = rows_by_rule(gpu_ctx, A, B, pairs, 16)
    want = ref.records(pairs, aln, cigar, n_cigar, queries, [0, 300])
    assert sum(r[2] for r in want) > ffi.SP_PILEUP_INS_LDS_RUNS and len(want) >= 12
    assert any(r[6] >= ffi.SP_ALIGN_PILEUP_SLICE for r in want) or any(int(n_cigar[i]) > 1 for i in range(ffi.SP_ALIGN_PILEUP_SLICE, n))
    got = gpu_ctx.align_pileup(A, B, pairs, band=64, retry_band=256, insertions=True)
    assert ref.as_rows(got[3]) == want
    check_against_cols(ref.as_rows(got[3]), got[1], [0, 300])
    assert ref.as_rows(gpu_ctx.pileup_ins(A, B, pairs, aln, cigar, n_cigar)) == want

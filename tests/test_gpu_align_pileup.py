"""sp_align_pileup_batch: align, pile up and summarise without the op rows leaving the device (sp_pileup.hip), held to the composition it replaces --
sp_affine_align_batch(band = 64, cigar_stride = 4096) + sp_pileup_batch + sp_support_summarize per target -- field by field, exactly, and to tests/pileup_ref.py.

One main batch, aligned once by both routes, covers the shapes at which the kernels take another path:
  targets   1, 63, 64, 65 (lane edges) and T - 1, T, T + 1, 2 T + 5 columns (tile edges; T = SP_PILEUP_TILE); a 65-column target that no pair names
  pairs     per target none, one, or nine (more than SP_PILEUP_WAVES); queries with substitutions, insertions and deletions of 1, 7 and 40 bases, an N, a row of more
            than 64 ops (the chunk carry), an alignment from one tile into the next, an 'I' op at a tile's first column; pairs that score 0: an all-N query, a query
            whose band misses the target, a pair switched off (max_ed < 0)
A second batch of SP_ALIGN_PILEUP_SLICE + 37 pairs on three targets runs in two slices with every target in both; a third holds designed depth profiles for the summary
kernel, one of them with 1,100 distinct depths: more than the SP_SUPPORT_HIST_BINS = 1,024 bins of its LDS histogram."""
import ctypes as C

import numpy as np
import pytest

import pileup_ref as pr

pytestmark = pytest.mark.gpu

BASES = "ACGT"


def rand_seq(rng, n):
    return "".join(BASES[i] for i in rng.integers(0, 4, n))


def substitute(seq, positions, shift=1):
    s = list(seq)
    for k, p in enumerate(positions):
        s[p] = BASES[(BASES.index(s[p]) + 1 + (k + shift) % 3) % 4]
    return "".join(s)


def composition(ctx, ffi, A, B, pairs, stride):
    """the route the new call replaces: (aln, cigar, n_cigar, [cols per target], [summary per target])"""
    aln, cigar, n_cigar = ctx.affine_align(A, B, pairs, a=1, band=64, cigar_stride=stride)
    assert n_cigar.max() <= stride
    cols = ctx.pileup(A, B, pairs, aln, cigar, n_cigar)
    sums = []
    for t in range(B.n):
        named = [i for i, p in enumerate(pairs) if p[1] == t]
        sums.append(ffi.support_summarize(cols[t], n_members=len(named), n_aligned=sum(int(aln[i]["score"]) > 0 for i in named)))
    return aln, cigar, n_cigar, cols, sums


def same_tables(got, want):
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), t
        bad = np.argwhere(pr.as_table(g) != pr.as_table(w))
        assert len(bad) == 0, (t, bad[:5])


@pytest.fixture(scope="module")
def batch(pkg, gpu_ctx):
    ffi = pkg.ffi
    T, W = ffi.SP_PILEUP_TILE, ffi.SP_PILEUP_WAVES
    rng = np.random.default_rng(1234)
    lens = [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 5, 65]                  # the last one gets no pair
    targets = [rand_seq(rng, n) for n in lens]
    queries, pairs = [], []

    def add(t, q, t_pos, q_pos=0, max_ed=0):                                # base q_pos of query q faces column t_pos of target t
        queries.append(q)
        pairs.append((len(queries) - 1, t, t_pos - q_pos, max_ed))

    add(0, targets[0], 0)                                                   # one pair on the one-column target
    add(1, targets[1], 0)                                                   # one pair, 63 columns
    for k in range(9):                                                      # nine pairs on 64 columns
        add(2, substitute(targets[2], [10 + 3 * k, 40 + k], shift=k), 0)
    add(3, substitute(targets[3], [31, 50]), 0)                             # 65 columns: a run into the one column behind the lane edge
    for k in range(9):                                                      # nine pairs, every one covering every column of the T - 1 target
        add(4, substitute(targets[4], range(30 + k, T - 40, 97 + k), shift=k), 0)
    t5 = targets[5]
    add(5, substitute(t5[5:1008], range(3, 1003, 7)), 5)                    # a mismatch every 7 bases: more than 64 ops
    add(5, t5[T - 531:T], T - 531)                                          # ends on the tile's last column
    add(5, t5[300:500] + "N" + t5[501:700], 300)                            # an N in the query
    add(5, "N" * 120, 900)                                                  # nothing but N: score 0
    add(5, t5[100:300], T + 400)                                            # the band misses the target: score 0
    add(5, t5[100:300], 100, max_ed=-1)                                     # switched off: score 0
    t6 = targets[6]
    add(6, substitute(t6[T - 700:], [100, 350, 688]), T - 700)              # into a second tile of exactly one column
    add(6, t6[T - 90:], T - 90)
    t7 = targets[7]
    add(7, substitute(t7[100:777], range(5, 670, 7), shift=2), 100)
    add(7, t7[T - 301:T - 3] + t7[T + 4:T + 300], T - 301 + 3)              # a 7-base deletion across the tile edge (the diagonal between both flanks)
    other = next(b for b in BASES if b not in (t7[T - 1], t7[T]))
    add(7, t7[T - 211:T] + other * 3 + t7[T:T + 190], T - 211)              # an 'I' op at the first column of tile 1
    add(7, t7[2 * T - 100:], 2 * T - 100)                                   # into the 5 columns of the third tile
    add(7, t7[T - 150:T + 150], T - 150)                                    # starts in tile 0, ends in tile 1
    add(7, t7[500:800] + rand_seq(rng, 40) + t7[800:1100], 500 - 20)        # a 40-base insertion
    add(7, t7[1200:1500] + t7[1540:1840], 1200 + 20)                        # a 40-base deletion
    add(7, t7[2300:2500] + other + t7[2500:2700], 2300)                     # a one-base insertion
    add(7, t7[3000:3200] + t7[3201:3400], 3000)                             # a one-base deletion
    A, B = gpu_ctx.upload(queries), gpu_ctx.upload(targets)
    aln, cigar, n_cigar, cols, sums = composition(gpu_ctx, ffi, A, B, pairs, 4096)
    got = gpu_ctx.align_pileup(A, B, pairs)
    return dict(ffi=ffi, T=T, W=W, lens=lens, targets=targets, queries=queries, A=A, B=B, pairs=pairs, aln=aln, cigar=cigar, n_cigar=n_cigar, cols=cols, sums=sums, got=got)


def runs_of(b, p):
    j, out = int(b["aln"][p]["b_start"]), []
    for k in range(int(b["n_cigar"][p])):
        op, n = int(b["cigar"][p][k]) & 15, int(b["cigar"][p][k]) >> 4
        out.append((op, j, n))
        if op != 1:
            j += n
    return out


def test_the_batch_holds_the_designed_cases(batch):
    b, T = batch, batch["T"]
    runs = [r for p in range(len(b["pairs"])) for r in runs_of(b, p)]
    assert max(b["n_cigar"]) > 64                                                                       # the chunk carry
    assert any(op == 1 and j == T for op, j, n in runs)                                                 # an 'I' op at a tile's first column
    assert any(op == 2 and j < T < j + n for op, j, n in runs)                                          # a deletion across a tile edge
    assert {n for op, j, n in runs if op == 1} >= {1, 3, 40} and {n for op, j, n in runs if op == 2} >= {1, 7, 40}
    assert any(int(a["b_start"]) < T < int(a["b_end"]) for a in b["aln"])                              # starts in one tile, ends in the next
    per_target = [sum(1 for p in b["pairs"] if p[1] == t) for t in range(len(b["lens"]))]
    assert per_target[8] == 0 and 1 in per_target and per_target.count(9) >= 2 and 9 > b["W"]
    zero = [i for i, a in enumerate(b["aln"]) if a["score"] == 0]
    assert len(zero) == 3 and all(b["pairs"][i][1] == 5 for i in zero)


def test_every_output_equals_the_composition(batch):
    b = batch
    aln, cols, sums = b["got"]
    assert aln.tobytes() == b["aln"].tobytes()
    same_tables(cols, b["cols"])
    assert sums == b["sums"]
    assert not cols[8].tobytes().strip(b"\0")                                                           # no pair names it
    assert sums[8] == dict(n_members=0, n_aligned=0, n_unaligned=0, length=65, min_depth=0, median_depth=0, n_contested=0)
    assert sums[5]["n_unaligned"] == 3 and sums[5]["n_aligned"] == 3
    assert (cols[4]["depth"] == 9).all()


def test_the_tables_equal_the_plain_python_statement(batch):
    b = batch
    ref = pr.pileup(b["queries"], b["lens"], b["pairs"], b["aln"], b["cigar"], b["n_cigar"])
    for t, tab in enumerate(ref):
        have = pr.as_table(b["got"][1][t])
        assert (have == tab).all(), t
        assert (have[:, 0] == have[:, 1] + have[:, 2:6].sum(axis=1) + have[:, 6]).all()
        named = [i for i, p in enumerate(b["pairs"]) if p[1] == t]
        n_al = sum(int(b["aln"][i]["score"]) > 0 for i in named)
        assert b["got"][2][t] == pr.summary(tab, len(named), n_al)
        assert list(b["ffi"].support_contested(b["got"][1][t])) == pr.contested(tab)


def test_outputs_that_are_not_asked_for(batch, gpu_ctx):
    b = batch
    aln, cols, sums = gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"], cols=False)
    assert cols is None and sums == b["sums"] and aln.tobytes() == b["aln"].tobytes()
    aln, cols, sums = gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"], aln=False, summaries=False)
    assert aln is None and sums is None
    same_tables(cols, b["cols"])
    members = [7 + t for t in range(len(b["lens"]))]                                                    # n_members is copied into the summaries
    sums = gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"], aln=False, cols=False, n_members=members)[2]
    assert [s["n_members"] for s in sums] == members
    assert [{k: v for k, v in s.items() if k != "n_members"} for s in sums] == [{k: v for k, v in s.items() if k != "n_members"} for s in b["sums"]]


def test_pair_order_does_not_matter(batch, gpu_ctx):
    b = batch
    order = list(np.random.default_rng(5).permutation(len(b["pairs"])))
    aln, cols, sums = gpu_ctx.align_pileup(b["A"], b["B"], [b["pairs"][i] for i in order])
    assert aln.tobytes() == b["aln"][np.array(order)].tobytes() and sums == b["sums"]
    same_tables(cols, b["cols"])


def test_a_warm_call_allocates_nothing(batch, gpu_ctx):
    b = batch
    gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"])
    before = gpu_ctx.profile_get("pool:device")
    again = gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"])
    assert gpu_ctx.profile_get("pool:device")[1:] == before[1:]
    assert again[0].tobytes() == b["aln"].tobytes() and again[2] == b["sums"]


def raw_call(b, gpu_ctx, rows, off):
    ffi = b["ffi"]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    aln = np.full(len(rows) * 6, 0x5A5A5A5A, np.uint32)
    cols = np.full(int(sum(b["lens"])) * 8, 0xABABABAB, np.uint32)
    sums = np.full(len(b["lens"]) * 8, 0xCDCDCDCD, np.uint32)
    op = ffi.sp_affine_opts(1, 4, 6, 2, 26, 1, 1)
    rc = ffi.lib().sp_align_pileup_batch(gpu_ctx._h, b["A"]._h, b["B"]._h, ptr(rows), len(rows), C.byref(op), ptr(off), ptr(aln), ptr(cols), ptr(sums), None)
    return rc, (aln == 0x5A5A5A5A).all() and (cols == 0xABABABAB).all() and (sums == 0xCDCDCDCD).all()


def test_bad_arguments_are_refused_before_any_launch(batch, gpu_ctx):
    b, ffi = batch, batch["ffi"]
    rows = np.zeros(len(b["pairs"]), ffi.PAIR_DTYPE)
    for i, p in enumerate(b["pairs"]):
        rows[i] = p
    off = np.zeros(len(b["lens"]) + 1, np.uint64)
    off[1:] = np.cumsum(b["lens"])
    launches = lambda: gpu_ctx.profile_get("align_pileup_map")[1]
    n0 = launches()
    for field, value in (("a", len(b["queries"])), ("b", len(b["lens"]))):
        bad = rows.copy()
        bad[3][field] = value
        rc, untouched = raw_call(b, gpu_ctx, bad, off)
        assert rc == ffi.SP_ERR_INVALID_ARG and untouched
        assert "out of range" in ffi.lib().sp_last_error(gpu_ctx._h).decode()
    wrong = off.copy()
    wrong[3] += 1                                                                                       # target 2 one column longer, target 3 one shorter
    rc, untouched = raw_call(b, gpu_ctx, rows, wrong)
    assert rc == ffi.SP_ERR_INVALID_ARG and untouched
    assert "col_offset" in ffi.lib().sp_last_error(gpu_ctx._h).decode()
    assert launches() == n0
    rc, untouched = raw_call(b, gpu_ctx, rows, off)                                                     # and the untouched batch still runs
    assert rc == ffi.SP_OK and not untouched


def test_a_batch_of_more_than_one_slice_adds_up(pkg, gpu_ctx):
    """SP_ALIGN_PILEUP_SLICE + 37 pairs of 150 - 300-base queries on three targets, dealt round robin: every target has pairs in both slices, and a tile that the
    first slice wrote is loaded, added to and stored by the second"""
    ffi = pkg.ffi
    S = ffi.SP_ALIGN_PILEUP_SLICE
    rng = np.random.default_rng(99)
    targets = [rand_seq(rng, n) for n in (300, 2500, 4200)]                                            # one, two and three tiles
    queries, pairs = [], []
    for i in range(S + 37):
        t = i % 3
        n = int(rng.integers(150, 301))
        lo = int(rng.integers(0, len(targets[t]) - n + 1))
        q = substitute(targets[t][lo:lo + n], sorted(rng.choice(np.arange(20, n - 20), 3, replace=False)), shift=i)
        if i % 5 == 0:
            q = q[:70] + q[72:]                                                                         # a two-base deletion
        queries.append(q)
        pairs.append((i, t, lo, 0))
    assert {p[1] for p in pairs[:S]} == {0, 1, 2} == {p[1] for p in pairs[S:]}
    A, B = gpu_ctx.upload(queries), gpu_ctx.upload(targets)
    aln, cigar, n_cigar, cols, sums = composition(gpu_ctx, ffi, A, B, pairs, 64)
    got = gpu_ctx.align_pileup(A, B, pairs)
    assert got[0].tobytes() == aln.tobytes() and (aln["score"] > 0).all()
    same_tables(got[1], cols)
    assert got[2] == sums
    assert gpu_ctx.align_pileup(A, B, pairs, aln=False, cols=False)[2] == sums


def test_designed_depth_profiles(pkg, gpu_ctx):
    """summary tables made by exact substrings of the target (every pair is one '=' run, so a column's depth is the number of queries over it):
      0  40 columns (even), prefixes of 10, 20, 30, 40 bases: a staircase          1  41 columns (odd), the same
      2  50 columns, three full-length copies: every column the same depth          3  40 columns, depth 2 on 20 columns and 1 on the other 20: a tie across the
         median -- the lower median is 1                                            4  1,200 columns, prefixes of 1 .. 1,100 bases: 1,100 distinct depths (1,101 with
         the 0 behind them), more than the 1,024 bins of the histogram: coarse bins and a second pass"""
    ffi = pkg.ffi
    bins = ffi.SP_SUPPORT_HIST_BINS
    assert bins == 1024
    rng = np.random.default_rng(4)
    targets = [rand_seq(rng, n) for n in (40, 41, 50, 40, 1200)]
    queries, pairs = [], []

    def add(t, lo, hi):
        queries.append(targets[t][lo:hi])
        pairs.append((len(queries) - 1, t, lo, 0))

    for t in (0, 1):
        for n in (10, 20, 30, len(targets[t])):
            add(t, 0, n)
    for _ in range(3):
        add(2, 0, 50)
    add(3, 0, 40)
    add(3, 0, 20)
    n_deep = 1100
    assert n_deep > bins
    for n in range(1, n_deep + 1):
        add(4, 0, n)
    A, B = gpu_ctx.upload(queries), gpu_ctx.upload(targets)
    aln, cigar, n_cigar, cols, sums = composition(gpu_ctx, ffi, A, B, pairs, 8)
    assert (n_cigar == 1).all() and (aln["score"] == [len(q) for q in queries]).all()
    got = gpu_ctx.align_pileup(A, B, pairs)
    same_tables(got[1], cols)
    assert got[2] == sums
    assert len(set(int(d) for d in cols[4]["depth"])) == n_deep + 1 > bins
    assert [(s["min_depth"], s["median_depth"]) for s in got[2]] == [(1, 2), (1, 2), (3, 3), (1, 1), (0, 500)]      # 100 zeros, then 1 .. 1,100: element 599
    assert all(s["n_contested"] == 0 for s in got[2])


def test_an_op_buffer_that_is_too_small_is_grown_and_the_slice_run_again(pkg, batch):
    """on a fresh context the op buffer starts at 64 words per pair; eight pairs of ~285 ops each ask for more, so the map is run a second time on a buffer of the size
    it asked for -- the same outputs as the composition, a larger pool afterwards, and a warm call that allocates nothing"""
    ffi = pkg.ffi
    ctx = pkg.Context(0)
    rng = np.random.default_rng(8)
    target = rand_seq(rng, 1100)
    queries = [substitute(target[5 + k:1008 + k], range(3, 1003, 7), shift=k) for k in range(8)]
    pairs = [(k, 0, 5 + k, 0) for k in range(8)]
    A, B = ctx.upload(queries), ctx.upload([target])
    aln, cigar, n_cigar, cols, sums = composition(ctx, ffi, A, B, pairs, 4096)
    assert int(n_cigar.sum()) > 64 * len(pairs)
    before = ctx.profile_get("pool:device")
    maps = ctx.profile_get("align_pileup_map")[1]
    got = ctx.align_pileup(A, B, pairs)
    assert ctx.profile_get("align_pileup_map")[1] == maps + 2                                          # the slice ran twice
    assert got[0].tobytes() == aln.tobytes() and got[2] == sums
    same_tables(got[1], cols)
    warm = ctx.profile_get("pool:device")
    assert warm[1] > before[1]
    again = ctx.align_pileup(A, B, pairs)
    assert ctx.profile_get("pool:device")[1:] == warm[1:] and ctx.profile_get("align_pileup_map")[1] == maps + 3
    assert again[0].tobytes() == aln.tobytes() and again[2] == sums
    ctx.close()

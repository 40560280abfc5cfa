"""sp_align_pileup_band_batch: the device-resident align-and-pileup pass on 256 diagonals, and on 64 with a second try on 256 (sp_pileup.hip; the map kernel with four
diagonals per lane, sp_affine.hip), held to the composition the library already trusts, run on the same pairs: sp_affine_align_batch(band, cigar_stride = 4096) +
sp_pileup_batch + sp_support_summarize per target -- field for field, exactly.

The wide batch, aligned once by both routes:
  targets   1, 63, 64, 65, 255, 256, 257 columns and R - 1, R, R + 1, 2 R + 1 rows (R = SP_ALIGN_PILEUP_WIDE_ROWS, the rows of a checkpoint block), and two long ones
  queries   clean copies, substitutions, an N, a 100-base deletion and a 100-base insertion in mid-read (the path leaves the centre 64 diagonals), a 5-base insertion
            whose F run starts on band index 4 k + 2 and crosses into the next lane's four diagonals, walks that cross a checkpoint block at row R (a plain one, one
            that begins on row R, one with a deletion over the block edge), a row of more than 64 ops, an all-N query, a pair switched off, a pair whose 256
            diagonals still miss the target
The retry batch holds pairs that align on 64 diagonals, pairs whose 64-diagonal rectangle is empty while the 256-diagonal one aligns, and pairs that align on neither."""
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


def summaries_of(ffi, B, pairs, aln, cols):
    sums = []
    for t in range(B.n):
        named = [i for i, p in enumerate(pairs) if p[1] == t]
        sums.append(ffi.support_summarize(cols[t], n_members=len(named), n_aligned=sum(int(aln[i]["score"]) > 0 for i in named)))
    return sums


def composition(ctx, ffi, A, B, pairs, band, stride=4096):
    """the yardstick at one band: (aln, cigar, n_cigar, [cols per target], [summary per target])"""
    aln, cigar, n_cigar = ctx.affine_align(A, B, pairs, a=1, band=band, cigar_stride=stride)
    assert n_cigar.max() <= stride
    cols = ctx.pileup(A, B, pairs, aln, cigar, n_cigar)
    return aln, cigar, n_cigar, cols, summaries_of(ffi, B, pairs, aln, cols)


def retry_composition(ctx, ffi, A, B, pairs, stride=4096):
    """the yardstick of the second try, pair by pair: band 64, then band 256 where that was attempted and gave score 0 or no ops
    -> (aln, [cols], [summaries], band_used, aln at 64, aln at 256)"""
    a64, c64, n64 = ctx.affine_align(A, B, pairs, a=1, band=64, cigar_stride=stride)
    a256, c256, n256 = ctx.affine_align(A, B, pairs, a=1, band=256, cigar_stride=stride)
    assert max(n64.max(), n256.max()) <= stride
    aln, cigar, n_cigar = a64.copy(), c64.copy(), n64.copy()
    used = np.zeros(len(pairs), np.uint32)
    for i, p in enumerate(pairs):
        again = p[3] >= 0 and (a64[i]["score"] <= 0 or n64[i] == 0)
        if again:
            aln[i], cigar[i], n_cigar[i] = a256[i], c256[i], n256[i]
        used[i] = 0 if aln[i]["score"] <= 0 or n_cigar[i] == 0 else (256 if again else 64)
    cols = ctx.pileup(A, B, pairs, aln, cigar, n_cigar)
    return aln, cols, summaries_of(ffi, B, pairs, aln, cols), used, a64, a256


def same_tables(got, want):
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), t
        bad = np.argwhere(pr.as_table(g) != pr.as_table(w))
        assert len(bad) == 0, (t, bad[:5])


@pytest.fixture(scope="module")
def wide(pkg, gpu_ctx):
    ffi = pkg.ffi
    R = ffi.SP_ALIGN_PILEUP_WIDE_ROWS
    rng = np.random.default_rng(4321)
    lens = [1, 63, 64, 65, 255, 256, 257, R - 1, R, R + 1, 2 * R + 1, 2000, 1300]
    targets = [rand_seq(rng, n) for n in lens]
    queries, pairs, tag = [], [], {}

    def add(t, q, diag, max_ed=0, name=None):
        queries.append(q)
        pairs.append((len(queries) - 1, t, diag, max_ed))
        if name:
            tag[name] = len(pairs) - 1

    for t in range(11):                                                     # a clean copy of every short target: every walk of more than R rows crosses a block
        add(t, targets[t], 0)
    for t in (4, 5, 6, 10):
        add(t, substitute(targets[t], range(7, lens[t] - 7, 29), shift=t), 0)
    tR1, t2R = targets[9], targets[10]
    add(9, tR1[R - 40:], R - 40, name="ends_on_row_R")                      # rows from 0 (diag < 128): the walk begins on row R, the one row of block 1
    add(10, t2R[R:], R, name="from_block_edge")
    add(10, t2R[:R - 3] + t2R[R + 2:], 0, name="deletion_over_block_edge")  # a 5-base deletion across rows R - 3 .. R + 1: the walk changes blocks inside a gap
    L = targets[11]
    add(11, L[200:500] + L[600:900], 200, name="del100")                    # the second flank lies 100 diagonals off
    add(11, L[1000:1300] + rand_seq(rng, 100) + L[1300:1600], 1000, name="ins100")
    other = next(b for b in BASES if b not in (L[1749], L[1750]))
    add(11, L[1600:1750] + other * 5 + L[1750:1900], 1600 + 2, name="ins5")  # given 2 off: the path runs on band index 128 + 2 = 4 k + 2, the gap on 131 .. 135
    add(11, L[300:700] + "N" + L[701:1000], 300)
    M = targets[12]
    add(12, substitute(M[5:1208], range(3, 1200, 7)), 5, name="many_ops")
    add(12, "N" * 150, 400, name="all_n")
    add(12, M[100:300], 100, max_ed=-1, name="off")
    add(12, M[100:300], lens[12] + 400, name="missed")                      # placed 400 columns behind the target's end: the 256 diagonals hold no cell
    A, B = gpu_ctx.upload(queries), gpu_ctx.upload(targets)
    aln, cigar, n_cigar, cols, sums = composition(gpu_ctx, ffi, A, B, pairs, 256)
    got = gpu_ctx.align_pileup(A, B, pairs, band=256, band_used=True)
    return dict(ffi=ffi, R=R, lens=lens, queries=queries, A=A, B=B, pairs=pairs, tag=tag, aln=aln, cigar=cigar, n_cigar=n_cigar, cols=cols, sums=sums, got=got)


def runs_of(b, p):
    return [(int(w) & 15, int(w) >> 4) for w in b["cigar"][p][:int(b["n_cigar"][p])]]


def test_the_wide_batch_holds_the_designed_cases(wide, gpu_ctx):
    b, tag, R = wide, wide["tag"], wide["R"]
    both = [tag["del100"], tag["ins100"]]
    narrow = gpu_ctx.affine_align(b["A"], b["B"], [b["pairs"][i] for i in both], a=1, band=64, cigar_stride=4096)[0]
    for k, i in enumerate(both):                                                                       # the 64 diagonals see one flank only
        assert narrow[k].tobytes() != b["aln"][i].tobytes() and b["aln"][i]["score"] > narrow[k]["score"] > 0
    assert (2, 100) in runs_of(b, tag["del100"]) and (1, 100) in runs_of(b, tag["ins100"])
    assert b["aln"][tag["del100"]]["a_end"] == 600 and b["aln"][tag["ins100"]]["a_end"] == 700
    assert (1, 5) in runs_of(b, tag["ins5"]) and b["aln"][tag["ins5"]]["b_start"] - b["aln"][tag["ins5"]]["a_start"] == 1600
    assert (2, 5) in runs_of(b, tag["deletion_over_block_edge"])
    assert b["aln"][tag["ends_on_row_R"]]["b_end"] == R + 1 and b["aln"][tag["from_block_edge"]]["b_start"] == R
    assert b["n_cigar"][tag["many_ops"]] > 64
    assert [int(b["aln"][tag[k]]["score"]) for k in ("all_n", "off")] == [0, 0] and b["n_cigar"][tag["missed"]] == 0
    assert all(b["aln"][t]["score"] == n for t, n in enumerate(b["lens"][:11]))                         # the clean copies, whole


def test_band_256_equals_the_composition(wide):
    b = wide
    aln, cols, sums, used = b["got"]
    assert aln.tobytes() == b["aln"].tobytes()
    same_tables(cols, b["cols"])
    assert sums == b["sums"]
    assert (used == np.where((b["aln"]["score"] > 0) & (b["n_cigar"] > 0), 256, 0)).all() and (used == 0).sum() == 3


def test_band_64_through_the_new_entry_is_the_old_call(wide, gpu_ctx):
    b = wide
    old = gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"])
    new = gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"], band=64, retry_band=0, band_used=True)
    assert new[0].tobytes() == old[0].tobytes() and new[2] == old[2]
    assert [c.tobytes() for c in new[1]] == [c.tobytes() for c in old[1]]
    assert (new[3] == np.where(old[0]["score"] > 0, 64, 0)).all()


@pytest.fixture(scope="module")
def retry(pkg, gpu_ctx):
    ffi = pkg.ffi
    rng = np.random.default_rng(77)
    targets = [rand_seq(rng, n) for n in (700, 2300)]
    queries, pairs = [], []

    def add(t, q, diag, max_ed=0):
        queries.append(q)
        pairs.append((len(queries) - 1, t, diag, max_ed))

    for t, tg in enumerate(targets):
        n = len(tg)
        for k in range(4):                                                  # align on 64 diagonals
            add(t, substitute(tg[50 + 9 * k:450 + 9 * k], [30, 200 + k, 333], shift=k), 50 + 9 * k)
        # 60-base queries whose true diagonal lies 80 off the one given: the 64-diagonal rectangle is empty, the 256-diagonal one holds the matching 30 bases
        add(t, tg[n - 30:] + rand_seq(rng, 30), n - 30 + 80)                # hangs over the target's end
        add(t, rand_seq(rng, 30) + tg[:30], -30 - 80)                       # hangs over its start
        add(t, tg[n - 25:] + rand_seq(rng, 35), n - 25 + 80)
        add(t, "N" * 90, 100)                                               # neither band: nothing but N
        add(t, tg[100:160], n + 400)                                        # neither band: both rectangles are empty
        add(t, tg[100:300], 100, max_ed=-1)                                 # switched off: never tried
    A, B = gpu_ctx.upload(queries), gpu_ctx.upload(targets)
    aln, cols, sums, used, a64, a256 = retry_composition(gpu_ctx, ffi, A, B, pairs)
    return dict(A=A, B=B, pairs=pairs, aln=aln, cols=cols, sums=sums, used=used, a64=a64, a256=a256)


def test_retry_equals_the_composition_pair_by_pair(retry, gpu_ctx):
    b = retry
    assert (b["used"] == 64).sum() == 8 and (b["used"] == 256).sum() == 6 and (b["used"] == 0).sum() == 6      # the three classes, from the composition alone
    assert all(b["a64"][i]["score"] == 0 and b["a256"][i]["score"] >= 25 for i in np.flatnonzero(b["used"] == 256))
    aln, cols, sums, used = gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"], band=64, retry_band=256, band_used=True)
    assert aln.tobytes() == b["aln"].tobytes()
    same_tables(cols, b["cols"])
    assert sums == b["sums"] and (used == b["used"]).all()
    assert gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"], aln=False, cols=False, retry_band=256)[2] == b["sums"]     # band_used is optional


def test_slices_with_retry_pairs_add_up(pkg, gpu_ctx):
    """SP_ALIGN_PILEUP_SLICE + 37 pairs on three targets, dealt round robin; every 41st pair is a retry pair (its 64-diagonal rectangle is empty): both slices hold some,
    every target is in both, and the retry list of the second slice starts from zero"""
    ffi = pkg.ffi
    S = ffi.SP_ALIGN_PILEUP_SLICE
    rng = np.random.default_rng(99)
    targets = [rand_seq(rng, n) for n in (300, 2500, 4200)]
    queries, pairs = [], []
    for i in range(S + 37):
        t = i % 3
        tg = targets[t]
        if i % 41 == 7:
            queries.append(tg[len(tg) - 40:] + rand_seq(rng, 30))
            pairs.append((i, t, len(tg) - 40 + 80, 0))
            continue
        n = int(rng.integers(150, 301))
        lo = int(rng.integers(0, len(tg) - n + 1))
        queries.append(substitute(tg[lo:lo + n], sorted(rng.choice(np.arange(20, n - 20), 3, replace=False)), shift=i))
        pairs.append((i, t, lo, 0))
    A, B = gpu_ctx.upload(queries), gpu_ctx.upload(targets)
    aln, cols, sums, used, a64, a256 = retry_composition(gpu_ctx, ffi, A, B, pairs, stride=64)
    for part in (used[:S], used[S:]):
        assert (part == 256).any() and (part == 64).any()
    assert {p[1] for p in pairs[:S]} == {0, 1, 2} == {p[1] for p in pairs[S:]} and (used > 0).all()
    got = gpu_ctx.align_pileup(A, B, pairs, band=64, retry_band=256, band_used=True)
    assert got[0].tobytes() == aln.tobytes()
    same_tables(got[1], cols)
    assert got[2] == sums and (got[3] == used).all()
    A.close()
    B.close()


def test_warm_calls_allocate_nothing(wide, retry, gpu_ctx):
    for b, kw in ((wide, dict(band=256)), (retry, dict(band=64, retry_band=256, band_used=True))):
        gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"], **kw)
        before = gpu_ctx.profile_get("pool:device")
        again = gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"], **kw)
        assert gpu_ctx.profile_get("pool:device")[1:] == before[1:]
        assert again[0].tobytes() == b["aln"].tobytes() and again[2] == b["sums"]


def test_band_arguments_are_refused_before_any_launch(wide, gpu_ctx):
    b, ffi = wide, wide["ffi"]
    rows = np.zeros(len(b["pairs"]), ffi.PAIR_DTYPE)
    for i, p in enumerate(b["pairs"]):
        rows[i] = p
    off = np.zeros(len(b["lens"]) + 1, np.uint64)
    off[1:] = np.cumsum(b["lens"])
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    op = ffi.sp_affine_opts(1, 4, 6, 2, 26, 1, 1)
    launches = lambda: sum(gpu_ctx.profile_get(n)[1] for n in ("align_pileup_map", "align_pileup_map_retry", "align_pileup_pile", "align_pileup_summary"))
    n0 = launches()
    for band, retry_band in ((128, 0), (64, 64), (256, 256)):
        aln = np.full(len(rows) * 6, 0x5A5A5A5A, np.uint32)
        cols = np.full(int(sum(b["lens"])) * 8, 0xABABABAB, np.uint32)
        sums = np.full(len(b["lens"]) * 8, 0xCDCDCDCD, np.uint32)
        used = np.full(len(rows), 0xEFEFEFEF, np.uint32)
        rc = ffi.lib().sp_align_pileup_band_batch(gpu_ctx._h, b["A"]._h, b["B"]._h, ptr(rows), len(rows), C.byref(op), band, retry_band, ptr(off), ptr(aln), ptr(cols), ptr(sums),
                                                  None, ptr(used))
        assert rc == ffi.SP_ERR_INVALID_ARG, (band, retry_band)
        assert (aln == 0x5A5A5A5A).all() and (cols == 0xABABABAB).all() and (sums == 0xCDCDCDCD).all() and (used == 0xEFEFEFEF).all()
        assert "band" in ffi.lib().sp_last_error(gpu_ctx._h).decode()
    assert launches() == n0

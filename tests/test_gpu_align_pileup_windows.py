"""sp_align_pileup_windows_batch: the window counts of the device-resident pass equal sp_pileup_windows_batch over the op rows sp_affine_align_batch returns for the
same pairs -- bit for bit, at band 64, at band 256 and at 64 with a second try on 256 --, windows == NULL is sp_align_pileup_band_batch, a batch of more than
SP_ALIGN_PILEUP_SLICE pairs accumulates across the slice boundary, and a second identical call allocates nothing."""
import numpy as np
import pytest

import pileup_win_ref as ref

pytestmark = pytest.mark.gpu

BASES = "ACGT"


def rand_seq(rng, n):
    return "".join(BASES[i] for i in rng.integers(0, 4, n))


def noisy(rng, s, n_edits):
    """s with n_edits substitutions, one-base insertions or one-base deletions at random places away from the ends"""
    s = list(s)
    for _ in range(n_edits):
        at = int(rng.integers(8, len(s) - 8))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            s[at] = BASES[(BASES.index(s[at]) + 1 + int(rng.integers(0, 3))) % 4]
        elif kind == 1:
            s.insert(at, BASES[int(rng.integers(0, 4))])
        else:
            del s[at]
    return "".join(s)


def windows_for(lens, rng, n_random):
    out = []
    for n in lens:
        w = [(j, j + k) for k in (1, 4, 9) for j in range(0, n - k, 7)] + [(0, n)]
        for _ in range(n_random):
            s = int(rng.integers(0, n - 1))
            w.append((s, int(rng.integers(s + 1, min(n, s + 60) + 1))))
        out.append(w)
    return out


def rows_by_rule(ctx, A, B, pairs, band, retry, stride=512):
    aln, cigar, n_cigar = ctx.affine_align(A, B, pairs, a=1, band=band, cigar_stride=stride)
    if retry:
        again = [i for i, p in enumerate(pairs) if p[3] >= 0 and (int(aln[i]["score"]) <= 0 or int(n_cigar[i]) == 0)]
        if again:
            aln2, cigar2, n2 = ctx.affine_align(A, B, [pairs[i] for i in again], a=1, band=retry, cigar_stride=stride)
            for k, i in enumerate(again):
                aln[i], cigar[i], n_cigar[i] = aln2[k], cigar2[k], n2[k]
    assert int(n_cigar.max()) <= stride
    return aln, cigar, n_cigar


@pytest.fixture(scope="module")
def batch(pkg, gpu_ctx):
    rng = np.random.default_rng(91)
    targets = [rand_seq(rng, 310), rand_seq(rng, 257), rand_seq(rng, 120), rand_seq(rng, 90)]          # target 3 gets no pair
    queries, pairs = [], []
    for t in (0, 1, 2):
        T = targets[t]
        for k in range(14):
            lo = int(rng.integers(0, len(T) // 3))
            hi = int(rng.integers(2 * len(T) // 3, len(T) + 1))
            queries.append(noisy(rng, T[lo:hi], int(rng.integers(0, 7))))
            pairs.append((len(queries) - 1, t, lo, 0))
    # a member whose 100-base insertion leaves the 64-diagonal band (the second try on 256 finds it), one that is switched off, one that is foreign
    T = targets[0]
    queries.append(T[20:150] + rand_seq(rng, 100) + T[150:300])
    pairs.append((len(queries) - 1, 0, 20, 0))
    queries.append(T[30:200])
    pairs.append((len(queries) - 1, 0, 30, -1))
    queries.append(rand_seq(rng, 150))
    pairs.append((len(queries) - 1, 1, 0, 0))
    A, B = gpu_ctx.upload(queries), gpu_ctx.upload(targets)
    return dict(ffi=pkg.ffi, A=A, B=B, pairs=pairs, windows=windows_for([len(t) for t in targets], rng, 40), lens=[len(t) for t in targets])


@pytest.mark.parametrize("band,retry", [(64, 0), (256, 0), (64, 256)])
def test_the_device_resident_form_equals_the_host_row_form(batch, gpu_ctx, band, retry):
    b = batch
    aln, cigar, n_cigar = rows_by_rule(gpu_ctx, b["A"], b["B"], b["pairs"], band, retry)
    want = gpu_ctx.pileup_windows(b["A"], b["B"], b["pairs"], aln, cigar, n_cigar, b["windows"])
    got = gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"], band=band, retry_band=retry, windows=b["windows"])
    assert got[0].tobytes() == aln.tobytes()
    assert [x.tobytes() for x in got[3]] == [x.tobytes() for x in want]
    # ... and the plain Python statement over the same rows
    alns = [(int(aln[i]["b_start"]), [int(w) for w in cigar[i, :int(n_cigar[i])]]) if int(n_cigar[i]) else None for i in range(len(b["pairs"]))]
    plain = ref.window_support([(p[0], p[1]) for p in b["pairs"]], alns, b["windows"])
    assert [[(int(r["span"]), int(r["exact"]), int(r["partial"])) for r in tab] for tab in got[3]] == plain
    assert any(r[1] < r[0] for tab in plain for r in tab) and any(r[1] for tab in plain for r in tab) and all(r == (0, 0, 0) for r in plain[3])
    # the table of the same call is the table of the call without windows
    base = gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"], band=band, retry_band=retry, band_used=True)
    assert base[0].tobytes() == got[0].tobytes() and base[2] == got[2] and [c.tobytes() for c in base[1]] == [c.tobytes() for c in got[1]]


def test_no_windows_is_the_band_call(batch, gpu_ctx):
    """windows == NULL, and a window list that is empty for every target: the outputs of sp_align_pileup_band_batch, byte for byte, and no window launch"""
    import ctypes as C
    b, ffi = batch, batch["ffi"]
    lib = ffi.lib()
    rows = np.zeros(len(b["pairs"]), ffi.PAIR_DTYPE)
    for i, p in enumerate(b["pairs"]):
        rows[i] = p
    off = np.zeros(len(b["lens"]) + 1, np.uint64)
    off[1:] = np.cumsum(b["lens"])
    op = ffi.sp_affine_opts(1, 4, 6, 2, 26, 1, 1)
    ptr = ffi._ptr

    def run(fn, *tail):
        aln = np.zeros(len(rows), ffi.AFFINE_DTYPE)
        cols = np.zeros(int(off[-1]), ffi.PILEUP_DTYPE)
        sums = np.zeros(len(b["lens"]), ffi.SUPPORT_DTYPE)
        gpu_ctx.check(fn(gpu_ctx._h, b["A"]._h, b["B"]._h, ptr(rows), len(rows), C.byref(op), 64, 256, ptr(off), ptr(aln), ptr(cols), ptr(sums), None, None, *tail))
        return aln.tobytes() + cols.tobytes() + sums.tobytes()
    want = run(lib.sp_align_pileup_band_batch)
    launches = gpu_ctx.profile_get("pileup_windows")[1]
    woff = np.zeros(len(b["lens"]) + 1, np.uint64)
    assert run(lib.sp_align_pileup_windows_batch, None, None, None) == want
    assert run(lib.sp_align_pileup_windows_batch, ptr(woff), ptr(np.zeros(1, ffi.WINDOW_DTYPE)), ptr(np.zeros(1, ffi.WINDOW_SUPPORT_DTYPE))) == want
    assert gpu_ctx.profile_get("pileup_windows")[1] == launches


def test_a_warm_call_allocates_nothing(batch, gpu_ctx):
    b = batch
    first = gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"], band=64, retry_band=256, windows=b["windows"])
    before = gpu_ctx.profile_get("pool:device")
    again = gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"], band=64, retry_band=256, windows=b["windows"])
    assert gpu_ctx.profile_get("pool:device")[1:] == before[1:]
    assert [x.tobytes() for x in again[3]] == [x.tobytes() for x in first[3]]


def test_bad_windows_are_refused_before_any_launch(pkg, batch, gpu_ctx):
    b = batch
    maps = gpu_ctx.profile_get("align_pileup_map")[1]
    for bad in ((4, 4), (0, b["lens"][0] + 1)):
        windows = [[bad]] + [[] for _ in b["lens"][1:]]
        with pytest.raises(pkg.StarphaseError) as e:
            gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"], windows=windows)
        assert e.value.code == pkg.ffi.SP_ERR_INVALID_ARG
    assert gpu_ctx.profile_get("align_pileup_map")[1] == maps


def test_a_batch_of_more_than_one_slice_accumulates(pkg, gpu_ctx):
    """SP_ALIGN_PILEUP_SLICE + 1 pairs of ~100 bases on three targets, dealt round robin: the last pair -- alone in the second slice -- is added to the records the
    first slice stored for its target, and the records of the two targets without a pair in that slice stay as they are"""
    ffi = pkg.ffi
    rng = np.random.default_rng(17)
    targets = [rand_seq(rng, 150), rand_seq(rng, 131), rand_seq(rng, 200)]
    distinct, pairs = [], []
    for t, T in enumerate(targets):                                          # 24 distinct members per target, repeated: the counts are large, the upload small
        for k in range(24):
            lo = int(rng.integers(0, len(T) - 100))
            distinct.append((noisy(rng, T[lo:lo + 100], int(rng.integers(0, 4))), t, lo))
    n = ffi.SP_ALIGN_PILEUP_SLICE + 1
    by_target = [[i for i, d in enumerate(distinct) if d[1] == t] for t in range(3)]
    for i in range(n):
        t = i % 3
        q = by_target[t][(i // 3) % 24]
        pairs.append((q, t, distinct[q][2], 0))
    A, B = gpu_ctx.upload([d[0] for d in distinct]), gpu_ctx.upload(targets)
    windows = windows_for([len(t) for t in targets], rng, 20)
    got = gpu_ctx.align_pileup(A, B, pairs, cols=False, summaries=False, windows=windows)
    aln, cigar, n_cigar = gpu_ctx.affine_align(A, B, [(q, distinct[q][1], distinct[q][2], 0) for q in range(len(distinct))], a=1, band=64, cigar_stride=256)
    alns = [(int(aln[q]["b_start"]), [int(w) for w in cigar[q, :int(n_cigar[q])]]) if int(n_cigar[q]) else None for q in range(len(distinct))]
    # the plain statement over all pairs: every distinct member's record times the number of pairs that repeat it
    times = np.bincount([p[0] for p in pairs], minlength=len(distinct))
    want = [[[0, 0, 0] for _ in w] for w in windows]
    for q in range(len(distinct)):
        one = ref.window_support([(q, distinct[q][1])], [alns[q]], windows)
        for t in range(3):
            for i, r in enumerate(one[t]):
                for k in range(3):
                    want[t][i][k] += int(times[q]) * r[k]
    assert [[(int(r["span"]), int(r["exact"]), int(r["partial"])) for r in tab] for tab in got[3]] == [[tuple(r) for r in w] for w in want]
    assert max(r[0] for w in want for r in w) > ffi.SP_ALIGN_PILEUP_SLICE // 3 - 50
    assert times.min() > 0 and int(times.sum()) == n

"""sp_pileup_hap_batch and sp_align_pileup_hap_batch (sp_pileup.hip): the distinct patterns of calls the member alignments make at the contested columns of their
target, held record for record and head for head to tests/pileup_hap_ref.py over the op rows of sp_affine_align_batch, and to the three invariants of the header
against the library's own column table.

One batch holds the designed targets: two linked haplotypes (three contested columns, two patterns, 12 and 10 reads); the same three edits scattered over the
members (many patterns); the linked pile with a member that ends before the second column (call 0); an 'X' facing an N of the query (call 2); contested columns 2047
and 2048 of a 5,000-base target (the pileup's tile edge); exactly 64 and 70 contested columns (the cap: n_cols 64, n_cols_total 70); a target no pair names and a target
without a contested column (no records).  Hand-made op rows put an 'I' behind column 0 and behind a member's last aligned column.  A batch of SP_ALIGN_PILEUP_SLICE + 1
members puts every kind of read into both slices and more keys on one target than the sort holds in LDS; one of its columns is contested only through the sum of
the slices (not inside the first: one member of that slice begins behind the column), so the calls of the first slice's rows are made after the last slice.  A batch
of the same size with more than 64 ops per pair, on a context of its own, overflows the cold op buffer behind the first slice: the rows kept move into a second buffer and that slice alone runs again."""
import ctypes as C

import numpy as np
import pytest

import pileup_hap_ref as ref

pytestmark = pytest.mark.gpu

BASES = "ACGT"


def rand_seq(rng, n):
    return "".join(BASES[i] for i in rng.integers(0, 4, n))


def other(base, k=0):
    return [b for b in BASES if b != base][k]


def sub(s, c, k=0):
    return s[:c] + other(s[c], k) + s[c + 1:]


def foreign(target, c):
    return [b for b in BASES if b not in (target[c], target[c + 1])]


def linked_target(rng):
    """600 bases; the base at 300 differs from both neighbours, so its deletion has one place"""
    t = list(rand_seq(rng, 600))
    t[299:302] = "ACG"
    return "".join(t)


def edited(t, x=False, d=False, i=False):
    """t with an X at column 100, a 1-base deletion at column 300, a 2-base insertion behind column 450 (applied from the right: the columns stay t's)"""
    s = t
    if i:
        s = s[:451] + foreign(t, 450)[0] * 2 + s[451:]
    if d:
        s = s[:300] + s[301:]
    if x:
        s = sub(s, 100)
    return s


def rows_by_rule(ctx, A, B, pairs, stride):
    """sp_affine_align_batch on 64 diagonals, and on 256 for the attempted pairs that came back with score 0 or without ops"""
    aln, cigar, n_cigar = ctx.affine_align(A, B, pairs, a=1, band=64, cigar_stride=stride)
    again = [i for i, p in enumerate(pairs) if p[3] >= 0 and (int(aln[i]["score"]) <= 0 or int(n_cigar[i]) == 0)]
    if again:
        aln2, cigar2, n2 = ctx.affine_align(A, B, [pairs[i] for i in again], a=1, band=256, cigar_stride=stride)
        for k, i in enumerate(again):
            aln[i], cigar[i], n_cigar[i] = aln2[k], cigar2[k], n2[k]
    assert int(n_cigar.max()) <= stride
    return aln, cigar, n_cigar


T_LINKED, T_NOISE, T_EDGE, T_UNNAMED, T_CALM, T_64, T_70, T_N, T_PARTIAL = range(9)


@pytest.fixture(scope="module")
def batch(pkg, gpu_ctx):
    ffi = pkg.ffi
    rng = np.random.default_rng(2025)
    linked = linked_target(rng)
    t_n = list(rand_seq(rng, 300))
    t_n[150] = "C"                                                                                     # an N is stored with code 0 (A): a mismatch either way
    targets = [linked, linked_target(rng), rand_seq(rng, 5000), rand_seq(rng, 400), rand_seq(rng, 300), rand_seq(rng, 64 * 20 + 20), rand_seq(rng, 70 * 20 + 20),
               "".join(t_n), linked]
    queries, pairs = [], []

    def add(t, q, diag=0):
        queries.append(q)
        pairs.append((len(queries) - 1, t, diag, 0))

    for t in (T_LINKED, T_PARTIAL):                                                                    # two linked haplotypes: 10 and 12 reads
        for _ in range(10):
            add(t, targets[t])
        for _ in range(12):
            add(t, edited(targets[t], True, True, True))
    add(T_PARTIAL, targets[T_PARTIAL][:250])                                                           # ends before column 300
    for i in range(24):                                                                                # the same edits, scattered
        add(T_NOISE, edited(targets[T_NOISE], i % 2 == 0, (i // 2) % 2 == 0, (i // 4) % 2 == 0 or i == 23))
    e = targets[T_EDGE]
    add(T_EDGE, e[1900:2200], 1900)
    add(T_EDGE, sub(sub(e, 2047), 2048)[1900:2200], 1900)
    for _ in range(2):
        add(T_CALM, targets[T_CALM])
    for t, k in ((T_64, 64), (T_70, 70)):                                                              # depth 2, eq 1 on every 20th column
        s = targets[t]
        add(t, s)
        for c in range(10, 20 * k, 20):
            s = sub(s, c, c % 3)
        add(t, s)
    n_t = targets[T_N]
    add(T_N, n_t)
    add(T_N, n_t[:150] + "N" + n_t[151:])
    A, B = gpu_ctx.upload(queries), gpu_ctx.upload(targets)
    lengths = [len(t) for t in targets]
    aln, cigar, n_cigar = rows_by_rule(gpu_ctx, A, B, pairs, 256)
    want = ref.records(pairs, aln, cigar, n_cigar, queries, lengths)
    got = gpu_ctx.align_pileup(A, B, pairs, band=64, retry_band=256, insertions=True, haplotypes=True)
    return dict(ffi=ffi, targets=targets, lengths=lengths, queries=queries, pairs=pairs, A=A, B=B, aln=aln, cigar=cigar, n_cigar=n_cigar, want=want, got=got)


def records_of(want, t):
    recs, heads, _ = want
    return recs[heads[t][0]:heads[t][0] + heads[t][1]]


def test_the_batch_holds_the_designed_cases(batch):
    want = batch["want"]
    recs, heads, tab = want
    assert heads[T_LINKED][1:] == (2, 3, 3) and ref.contested(tab[T_LINKED]) == [100, 300, 450]
    a, b = records_of(want, T_LINKED)
    assert (a[2], b[2]) == (12, 10) and ref.text(b) == "===" and ref.text(a)[1:] == "-=+" and ref.text(a)[0] in "ACGT"
    assert heads[T_NOISE][2] == 3 and heads[T_NOISE][1] >= 8
    assert "=??" in [ref.text(r) for r in records_of(want, T_PARTIAL)] and heads[T_PARTIAL][1] == 3
    assert ref.contested(tab[T_EDGE]) == [2047, 2048] and heads[T_EDGE][1] == 2
    assert heads[T_UNNAMED][1:] == (0, 0, 0) and heads[T_CALM][1:] == (0, 0, 0)
    assert heads[T_64][1:] == (2, 64, 64) and heads[T_70][1:] == (2, 64, 70)
    assert ref.contested(tab[T_N]) == [150] and sorted(ref.call(r, 0) for r in records_of(want, T_N)) == [1, 2]      # the N is an 'X' with code 0: call 2


def test_the_host_rows_call_equals_the_reference(batch, gpu_ctx):
    b = batch
    haps, heads = gpu_ctx.pileup_hap(b["A"], b["B"], b["pairs"], b["aln"], b["cigar"], b["n_cigar"])
    assert ref.as_rows(haps) == b["want"][0] and ref.as_heads(heads) == b["want"][1]
    ref.check_invariants(ref.as_rows(haps), ref.as_heads(heads), gpu_ctx.pileup(b["A"], b["B"], b["pairs"], b["aln"], b["cigar"], b["n_cigar"]))
    for r, row in zip(haps, ref.as_rows(haps)):
        assert b["ffi"].support_hap_string(r) == ref.text(row)


def test_the_device_resident_call_equals_the_reference(batch):
    b = batch
    aln, cols, sums, ins, (haps, heads) = b["got"]
    assert aln.tobytes() == b["aln"].tobytes()
    assert ref.as_rows(haps) == b["want"][0] and ref.as_heads(heads) == b["want"][1]
    ref.check_invariants(ref.as_rows(haps), ref.as_heads(heads), cols, [s["n_aligned"] for s in sums])


def test_the_device_resident_call_on_256_diagonals(batch, gpu_ctx):
    b = batch
    aln, cigar, n_cigar = gpu_ctx.affine_align(b["A"], b["B"], b["pairs"], a=1, band=256, cigar_stride=256)
    assert int(n_cigar.max()) <= 256
    want = ref.records(b["pairs"], aln, cigar, n_cigar, b["queries"], b["lengths"])
    got = gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"], band=256, haplotypes=True)
    assert ref.as_rows(got[3][0]) == want[0] and ref.as_heads(got[3][1]) == want[1]
    host = gpu_ctx.pileup_hap(b["A"], b["B"], b["pairs"], aln, cigar, n_cigar)
    assert host[0].tobytes() == got[3][0].tobytes() and host[1].tobytes() == got[3][1].tobytes()


def test_the_list_does_not_depend_on_the_order_of_the_pairs(batch, gpu_ctx):
    b = batch
    perm = np.random.default_rng(3).permutation(len(b["pairs"]))
    pairs = [b["pairs"][int(i)] for i in perm]
    aln, cigar, n_cigar = b["aln"][perm], b["cigar"][perm], b["n_cigar"][perm]
    want = ref.records(pairs, aln, cigar, n_cigar, b["queries"], b["lengths"])
    strip = lambda rows: [r[:3] + r[4:] for r in rows]
    assert strip(want[0]) == strip(b["want"][0]) and want[1] == b["want"][1]
    assert [r[3] for r in want[0]] != [r[3] for r in b["want"][0]]                                     # first_pair follows the caller's indices
    haps, heads = gpu_ctx.pileup_hap(b["A"], b["B"], pairs, aln, cigar, n_cigar)
    assert ref.as_rows(haps) == want[0] and ref.as_heads(heads) == want[1]
    got = gpu_ctx.align_pileup(b["A"], b["B"], pairs, band=64, retry_band=256, haplotypes=True)
    assert ref.as_rows(got[3][0]) == want[0] and ref.as_heads(got[3][1]) == want[1]


def test_without_the_list_the_neighbouring_outputs_are_the_same_bytes(batch, gpu_ctx):
    b, ffi = batch, batch["ffi"]
    aln, cols, sums, ins, (haps, heads) = b["got"]
    launches = gpu_ctx.profile_get("support_hap")[1]
    pool = gpu_ctx.profile_get("pool:device")
    old = gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"], band=64, retry_band=256, insertions=True)
    assert old[0].tobytes() == aln.tobytes() and old[2] == sums and old[3].tobytes() == ins.tobytes()
    assert all(o.tobytes() == c.tobytes() for o, c in zip(old[1], cols))
    # haps == NULL is sp_align_pileup_ins_batch: nothing else is launched, no further pool memory is taken
    rows = np.zeros(len(b["pairs"]), ffi.PAIR_DTYPE)
    for i, pr in enumerate(b["pairs"]):
        rows[i] = pr
    off = np.zeros(b["B"].n + 1, np.uint64)
    off[1:] = np.cumsum(b["lengths"])
    out = np.zeros(len(rows), ffi.AFFINE_DTYPE)
    table = np.zeros(int(off[-1]), ffi.PILEUP_DTYPE)
    sm = np.zeros(b["B"].n, ffi.SUPPORT_DTYPE)
    op = ffi.sp_affine_opts(1, 4, 6, 2, 26, 1, 1)
    rc = ffi.lib().sp_align_pileup_hap_batch(gpu_ctx._h, b["A"]._h, b["B"]._h, ffi._ptr(rows), len(rows), C.byref(op), 64, 256, ffi._ptr(off), ffi._ptr(out), ffi._ptr(table),
                                             ffi._ptr(sm), None, None, None, 0, None, None, 0, None, None)
    assert rc == ffi.SP_OK and gpu_ctx.profile_get("support_hap")[1] == launches and gpu_ctx.profile_get("pool:device")[1:] == pool[1:]
    assert out.tobytes() == aln.tobytes() and table.tobytes() == np.concatenate(cols).tobytes()


def test_a_warm_call_allocates_nothing(batch, gpu_ctx):
    b = batch
    gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"], band=64, retry_band=256, insertions=True, haplotypes=True)
    before = gpu_ctx.profile_get("pool:device")
    again = gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"], band=64, retry_band=256, insertions=True, haplotypes=True)
    assert gpu_ctx.profile_get("pool:device")[1:] == before[1:]
    assert again[4][0].tobytes() == b["got"][4][0].tobytes() and again[4][1].tobytes() == b["got"][4][1].tobytes()
    gpu_ctx.pileup_hap(b["A"], b["B"], b["pairs"], b["aln"], b["cigar"], b["n_cigar"])
    warm = gpu_ctx.profile_get("pool:device")
    gpu_ctx.pileup_hap(b["A"], b["B"], b["pairs"], b["aln"], b["cigar"], b["n_cigar"])
    assert gpu_ctx.profile_get("pool:device")[1:] == warm[1:]


def test_a_list_one_record_short_is_asked_for_again(batch, gpu_ctx):
    b, ffi = batch, batch["ffi"]
    n = len(b["want"][0])
    rc, haps, n_haps, heads = gpu_ctx.pileup_hap(b["A"], b["B"], b["pairs"], b["aln"], b["cigar"], b["n_cigar"], hap_cap=n - 1)
    assert rc == ffi.SP_ERR_CAPACITY and n_haps == n and haps is None
    rc, haps, n_haps, heads = gpu_ctx.pileup_hap(b["A"], b["B"], b["pairs"], b["aln"], b["cigar"], b["n_cigar"], hap_cap=n)
    assert rc == ffi.SP_OK and ref.as_rows(haps) == b["want"][0] and ref.as_heads(heads) == b["want"][1]
    res = gpu_ctx.align_pileup(b["A"], b["B"], b["pairs"], band=64, retry_band=256, insertions=True, haplotypes=True, hap_cap=n - 1)
    assert res[4] == (ffi.SP_ERR_CAPACITY, None, n, None)
    assert res[0].tobytes() == b["aln"].tobytes() and res[3].tobytes() == b["got"][3].tobytes()       # everything else is complete
    assert all(o.tobytes() == c.tobytes() for o, c in zip(res[1], b["got"][1]))


def test_hand_made_rows_behind_column_0_and_behind_a_members_last_column(pkg, gpu_ctx):
    ffi = pkg.ffi
    rng = np.random.default_rng(5)
    target = rand_seq(rng, 300)
    queries = [target[0] + "GAT" + target[1:120], target[50:150] + "CC", target[0] + "GAT" + target[1:100]]
    pairs = [(0, 0, 0, 0), (1, 0, 50, 0), (2, 0, 0, 0)]
    aln = np.zeros(3, ffi.AFFINE_DTYPE)
    aln[0] = (1, 0, 0, 123, 0, 120)
    aln[1] = (1, 0, 0, 102, 50, 150)
    aln[2] = (1, 0, 0, 103, 0, 100)
    cigar = np.zeros((3, 4), np.uint32)
    cigar[0, :3] = [(1 << 4) | 7, (3 << 4) | 1, (119 << 4) | 7]
    cigar[1, :2] = [(100 << 4) | 7, (2 << 4) | 1]
    cigar[2, :3] = [(1 << 4) | 7, (3 << 4) | 1, (99 << 4) | 7]
    n_cigar = np.array([3, 2, 3], np.uint32)
    A, B = gpu_ctx.upload(queries), gpu_ctx.upload([target])
    haps, heads = gpu_ctx.pileup_hap(A, B, pairs, aln, cigar, n_cigar)
    want = ref.records(pairs, aln, cigar, n_cigar, queries, [300])
    assert ref.as_rows(haps) == want[0] and ref.as_heads(heads) == want[1]
    assert ref.contested(want[2][0]) == [0, 149]
    assert [(r[2], r[3], ref.text(r)) for r in want[0]] == [(2, 0, "=+?"), (1, 1, "?=+")]
    ref.check_invariants(want[0], want[1], gpu_ctx.pileup(A, B, pairs, aln, cigar, n_cigar))


def test_more_pairs_than_a_slice_and_more_keys_than_lds_holds(pkg, gpu_ctx):
    ffi = pkg.ffi
    S = ffi.SP_ALIGN_PILEUP_SLICE
    n = S + 1
    assert n > ffi.SP_SUPPORT_HAP_LDS_KEYS and S % 2 == 0
    rng = np.random.default_rng(8)
    target = rand_seq(rng, 300)
    base = target[60:180]
    made = {}
    queries, pairs = [], []
    for i in range(n):
        # X at column 150 / at column 120: every kind in both slices.  Column 100: in the first slice the even members match (S / 2), the odd ones but one carry an X
        # (S / 2 - 1) and member 7 begins behind it -- 2 eq = S > S - 1 = depth, NOT contested; the one member of the second slice carries the X: 2 eq = S = depth
        kind = (i % 3 != 0, i % 5 < 3, i % 2 == 1 or i == S, i == 7)
        if kind not in made:
            q = base
            q = sub(q, 150 - 60) if kind[0] else q
            q = sub(q, 120 - 60) if kind[1] else q
            q = sub(q, 100 - 60) if kind[2] else q
            made[kind] = q[41:] if kind[3] else q
        queries.append(made[kind])
        pairs.append((i, 0, 101 if kind[3] else 60, 0))
    A, B = gpu_ctx.upload(queries), gpu_ctx.upload([target])
    aln, cigar, n_cigar = rows_by_rule(gpu_ctx, A, B, pairs, 16)
    want = ref.records(pairs, aln, cigar, n_cigar, queries, [300])
    first = ref.records(pairs[:S], aln[:S], cigar[:S], n_cigar[:S], queries, [300])
    assert ref.contested(first[2][0]) == [120, 150] and ref.contested(want[2][0]) == [100, 120, 150]      # column 100 is contested only through the sum
    c100 = want[2][0][100]
    assert (c100[0], c100[1]) == (S, S // 2) and (first[2][0][100][0], first[2][0][100][1]) == (S - 1, S // 2)
    assert want[1] == [(0, len(want[0]), 3, 3)] and len(want[0]) >= 8 and "?" in [ref.text(r)[0] for r in want[0]]
    before = None
    for _ in range(2):                                                                                 # (the second call is warm: no further pool memory)
        got = gpu_ctx.align_pileup(A, B, pairs, band=64, retry_band=256, haplotypes=True)
        assert ref.as_rows(got[3][0]) == want[0] and ref.as_heads(got[3][1]) == want[1]
        ref.check_invariants(want[0], want[1], got[1], [got[2][0]["n_aligned"]])
        now = gpu_ctx.profile_get("pool:device")[1:]
        assert before is None or now == before
        before = now
    plain = gpu_ctx.align_pileup(A, B, pairs, band=64, retry_band=256)
    assert plain[0].tobytes() == got[0].tobytes() and plain[1][0].tobytes() == got[1][0].tobytes() and plain[2] == got[2]
    host = gpu_ctx.pileup_hap(A, B, pairs, aln, cigar, n_cigar)
    assert ref.as_rows(host[0]) == want[0] and ref.as_heads(host[1]) == want[1]


def test_a_cold_op_buffer_too_small_for_the_batch_keeps_its_rows(pkg):
    """SP_ALIGN_PILEUP_SLICE + 1 members of 400 bases with an X every tenth base: 81 ops per pair, more than the 64 per pair a cold context guesses for the batch.  The
    first slice alone asks for a larger buffer (as without the list); the second then finds that one full: the rows kept move into the context's second op buffer and only
    that slice runs again.  The result is the reference's; a warm call launches each slice once and allocates nothing."""
    ffi = pkg.ffi
    ctx = pkg.Context(0)                                                                               # (its own pools: the op buffer is cold whatever ran before)
    n = ffi.SP_ALIGN_PILEUP_SLICE + 1
    rng = np.random.default_rng(12)
    target = rand_seq(rng, 400)
    marked = target
    for c in range(5, 400, 10):
        marked = sub(marked, c)
    queries = [marked if i % 2 else sub(marked, 200) for i in range(n)]                                 # column 200: half the members match, half carry an X
    pairs = [(i, 0, 0, 0) for i in range(n)]
    A, B = ctx.upload(queries), ctx.upload([target])
    aln, cigar, n_cigar = ctx.affine_align(A, B, pairs, a=1, band=64, cigar_stride=128)
    assert int(n_cigar.min()) > 64 and int(n_cigar.max()) <= 128 and int(aln["score"].min()) > 0
    want = ref.records(pairs, aln, cigar, n_cigar, queries, [400])
    assert want[1][0][3] >= 40 and len(want[0]) == 2
    cold = ctx.align_pileup(A, B, pairs, haplotypes=True)
    maps_cold = ctx.profile_get("align_pileup_map")[1]
    assert ref.as_rows(cold[3][0]) == want[0] and ref.as_heads(cold[3][1]) == want[1]
    ref.check_invariants(want[0], want[1], cold[1], [cold[2][0]["n_aligned"]])
    pool = ctx.profile_get("pool:device")[1:]
    warm = ctx.align_pileup(A, B, pairs, haplotypes=True)
    maps_warm = ctx.profile_get("align_pileup_map")[1] - maps_cold
    assert maps_warm == 2 and maps_cold == 4                                                    # one launch per slice when warm; cold, each slice ran twice
    assert ctx.profile_get("pool:device")[1:] == pool
    assert warm[0].tobytes() == cold[0].tobytes() and warm[3][0].tobytes() == cold[3][0].tobytes() and warm[1][0].tobytes() == cold[1][0].tobytes()
    A.close()
    B.close()
    ctx.close()

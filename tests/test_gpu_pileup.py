"""sp_pileup_batch: many alignments -> counts per target column (sp_pileup.hip), held to tests/pileup_ref.py field by field, exactly.

One batch, built and aligned once (sp_affine_align_batch on 64 diagonals, in this module), covers the shapes at which the kernel takes another path:
  targets   1, 63, 64, 65 (lane edges) and T - 1, T, T + 1, 2 T + 5 columns (tile edges; T = SP_PILEUP_TILE), every one with pairs; a second 2 T + 5 target for a pile
            across both tile edges; a 65- and a T + 1-column target that no pair names
  pairs     none (all-zero tables), one, 3 x waves + 1 on one target (every one covering all of its columns: depth == pairs), a mix elsewhere
  runs      queries with an edit planted every 7 bases (more than 64 and more than 128 ops: several chunks of the wave-wide prefix sum), a deletion that starts in
            the last columns of tile 0 and ends in tile 1, an insertion exactly behind the last column of tile 0, alignments that begin and end inside the target
  X bases   all four bases at planted mismatches; query lengths that are no multiple of 16 or 32
Two pairs carry hand-made ops instead of the aligner's: the aligner's local alignment never begins or ends on a mismatch (it clips there), so an X on the first and
on the last column of an alignment -- which the primitive must count like any other -- is written by hand, as is the one-column alignment on the one-column target."""
import ctypes as C

import numpy as np
import pytest

import pileup_hap_ref as hap_ref
import pileup_ins_ref as ins_ref
import pileup_ref as pr

pytestmark = pytest.mark.gpu

BASES = "ACGT"
STRIDE = 1024


def rand_seq(rng, n):
    return "".join(BASES[i] for i in rng.integers(0, 4, n))


def substitute(seq, positions, shift=1):
    s = list(seq)
    for k, p in enumerate(positions):
        s[p] = BASES[(BASES.index(s[p]) + 1 + (k + shift) % 3) % 4]         # the three other bases in turn
    return "".join(s)


@pytest.fixture(scope="module")
def batch(pkg, gpu_ctx):
    ffi = pkg.ffi
    T, W = ffi.SP_PILEUP_TILE, ffi.SP_PILEUP_WAVES
    rng = np.random.default_rng(77)
    lens = [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 5, 2 * T + 5, 65, T + 1]   # the last two get no pair: all-zero tables
    targets = [rand_seq(rng, n) for n in lens]
    queries, rows = [], []

    def add(t, q, t_pos):                                                   # query q lies on target t from column t_pos on
        queries.append(q)
        rows.append((len(queries) - 1, t, t_pos))

    add(1, targets[1], 0)                                                   # one pair on the 63-column target
    add(2, substitute(targets[2], [20, 41]), 0)
    add(3, substitute(targets[3], [31, 50]), 0)                             # 65 columns: a run into the one column behind the lane edge
    t6 = targets[6]
    add(6, substitute(t6[T - 700:], [100, 350, 688]), T - 700)              # T + 1 columns: runs that cross into a second tile of exactly one column
    add(6, t6[T - 90:], T - 90)
    for k in range(3 * W + 1):                                              # more pairs than waves, each covering every column of the T - 1 target
        add(4, substitute(targets[4], range(30 + k, T - 40, 97 + k), shift=k), 0)
    t5 = targets[5]
    add(5, substitute(t5[5:1008], range(3, 1003, 7)), 5)                    # 1,003 bases, a mismatch every 7: ~285 ops
    add(5, t5[T - 531:T], T - 531)                                          # ends on the tile's (and the target's) last column
    t7 = targets[7]
    add(7, substitute(t7[100:777], range(5, 670, 7), shift=2), 100)         # 677 bases: > 128 ops
    add(7, t7[T - 301:T - 3] + t7[T + 4:T + 300], T - 301)                  # a 7-base deletion across the tile edge
    other = next(b for b in BASES if b not in (t7[T - 1], t7[T]))
    add(7, t7[T - 211:T] + other * 3 + t7[T:T + 190], T - 211)              # an insertion exactly behind the last column of tile 0
    add(7, t7[2 * T - 100:], 2 * T - 100)                                   # into the 5 columns of the third tile
    add(7, substitute(t7[T - 50:T + 50], [37, 50, 63]), T - 50)
    t8 = targets[8]
    for k in range(6):                                                      # a pile across both tile edges of the second long target
        lo = 1500 + 131 * k
        add(8, substitute(t8[lo:lo + 1201 + k], range(11 + k, 1190, 61 + k), shift=k), lo)
    queries.append(substitute(targets[2][:63], [0, 62]))                    # the query of a hand-made pair below
    A, B = gpu_ctx.upload(queries), gpu_ctx.upload(targets)
    pairs = [(a, b, d) for a, b, d in rows]
    aln, cigar, n_cigar = gpu_ctx.affine_align(A, B, pairs, a=1, band=64, cigar_stride=STRIDE)
    assert (aln["score"] > 0).all() and n_cigar.max() <= STRIDE
    # the hand-made pairs: the first 63 columns of target 2 with the first and the last base substituted -- an X on the first and the last column of the alignment ...
    hq = len(queries) - 1
    hand = [((hq, 2, 0), (0, 2, 0, 63, 0, 63), [(1 << 4) | 8, (61 << 4) | 7, (1 << 4) | 8]),
            ((1, 0, 0), (1, 0, 0, 1, 0, 1), [(1 << 4) | (7 if queries[1][0] == targets[0] else 8)])]       # ... and one column on the one-column target
    for row, rec, words in hand:
        pairs.append(row)
        aln = np.append(aln, np.array([rec], aln.dtype))
        line = np.zeros((1, STRIDE), np.uint32)
        line[0, :len(words)] = words
        cigar = np.vstack([cigar, line])
        n_cigar = np.append(n_cigar, np.uint32(len(words)))
    ref = pr.pileup(queries, lens, pairs, aln, cigar, n_cigar)
    got = gpu_ctx.pileup(A, B, pairs, aln, cigar, n_cigar)
    return dict(ffi=ffi, T=T, W=W, lens=lens, targets=targets, queries=queries, A=A, B=B, pairs=pairs, aln=aln, cigar=cigar, n_cigar=n_cigar, ref=ref, got=got)


def runs_of(b, p):
    """(op, first target column, length) of every op of pair p"""
    j, out = int(b["aln"][p]["b_start"]), []
    for k in range(int(b["n_cigar"][p])):
        op, n = int(b["cigar"][p][k]) & 15, int(b["cigar"][p][k]) >> 4
        out.append((op, j, n))
        if op != 1:
            j += n
    return out


def test_the_batch_holds_the_designed_cases(batch):
    b, T = batch, batch["T"]
    per_pair = [runs_of(b, p) for p in range(len(b["pairs"]))]
    assert max(b["n_cigar"]) > 128 and sum(n > 64 for n in b["n_cigar"]) >= 2                           # several chunks
    on7 = [r for p, runs in enumerate(per_pair) if b["pairs"][p][1] == 7 for r in runs]
    assert any(op == 2 and j < T < j + n and j >= T - 8 for op, j, n in on7)                            # a deletion from the last columns of tile 0 into tile 1
    assert any(op == 1 and j == T for op, j, n in on7)                                                  # an insertion behind column T - 1
    assert any(runs[0][0] == 8 and runs[-1][0] == 8 for runs in per_pair)                               # X on the first and last column of an alignment
    inside = [(int(a["b_start"]), int(a["b_end"]), b["lens"][b["pairs"][p][1]]) for p, a in enumerate(b["aln"])]
    assert any(s > 0 and e < n for s, e, n in inside)                                                   # begins and ends inside its target
    assert any(len(q) % 16 and len(q) % 32 for q in b["queries"])
    x_total = sum(tab[:, 2:6].sum(axis=0) for tab in b["ref"])
    assert (x_total > 0).all()                                                                          # all four bases at mismatches


def test_every_field_equals_the_reference(batch):
    b = batch
    assert len(b["got"]) == len(b["lens"])
    for t, (got, ref) in enumerate(zip(b["got"], b["ref"])):
        assert len(got) == b["lens"][t]
        have = pr.as_table(got)
        bad = np.argwhere(have != ref)
        assert len(bad) == 0, (t, b["lens"][t], bad[:5], have[bad[:5, 0]], ref[bad[:5, 0]])
    for t in (9, 10):                                                                                   # no pair names them
        assert not b["got"][t].tobytes().strip(b"\0")
    assert (b["got"][4]["depth"] == 3 * b["W"] + 1).all()                                               # every pair covers every column
    assert b["got"][0]["depth"][0] == 1
    assert b["got"][3]["depth"][64] == 1 and b["got"][6]["depth"][b["T"]] == 2                          # real counts in the column behind the lane edge / in the one-column tile


def test_invariants(batch):
    b = batch
    eq_len = [0] * len(b["lens"])
    for p in range(len(b["pairs"])):
        eq_len[b["pairs"][p][1]] += sum(n for op, _, n in runs_of(b, p) if op == 7)
    for t, got in enumerate(b["got"]):
        tab = pr.as_table(got)
        assert (tab[:, 0] == tab[:, 1] + tab[:, 2:6].sum(axis=1) + tab[:, 6]).all(), t
        assert int(tab[:, 1].sum()) == eq_len[t], t


def test_determinism_and_pair_order(batch, gpu_ctx):
    b = batch
    flat = lambda tabs: b"".join(t.tobytes() for t in tabs)
    first = flat(b["got"])
    assert flat(gpu_ctx.pileup(b["A"], b["B"], b["pairs"], b["aln"], b["cigar"], b["n_cigar"])) == first
    n = len(b["pairs"])
    for order in (list(range(n))[::-1], list(np.random.default_rng(5).permutation(n))):
        o = np.array(order)
        again = gpu_ctx.pileup(b["A"], b["B"], [b["pairs"][i] for i in order], b["aln"][o], b["cigar"][o], b["n_cigar"][o])
        assert flat(again) == first


def test_host_rows_count_every_pair_with_ops_whatever_its_score(pkg, gpu_ctx):
    """The host-row entry points (pileup, pileup_ins, pileup_hap) count a pair when it has ops; its score is not looked at.  Hand-made rows, no aligner: targets of
    1, 65 and T + 1 columns, '=' 'X' 'I' 'D' rows (one crosses the tile edge, one has its 'I' behind the tile's last column), one pair without ops."""
    T = pkg.ffi.SP_PILEUP_TILE
    rng = np.random.default_rng(99)
    lens = [1, 65, T + 1]
    targets = [rand_seq(rng, n) for n in lens]
    plan = [(0, 0, [(8, 1)]),
            (0, 0, [(7, 1)]),
            (1, 0, [(7, 20), (8, 1), (7, 10), (1, 3), (7, 33), (8, 1)]),                                # all 65 columns, an X on the last
            (1, 0, [(7, 20), (8, 1), (7, 10), (1, 3), (7, 34)]),                                        # the same insertion once more
            (1, 5, [(7, 10), (2, 4), (7, 6), (8, 1), (7, 20)]),
            (2, T - 30, [(7, 20), (2, 10), (8, 1)]),                                                    # a deletion up to the tile edge, an X in the one-column tile
            (2, T - 5, [(7, 3), (8, 1), (7, 1), (1, 2), (8, 1)]),                                       # an insertion behind the last column of tile 0
            (2, 0, [(8, 1), (7, 99), (1, 1), (7, 50), (2, 2), (8, 2), (7, 10)]),
            (2, T - 30, [(7, 20), (8, 1), (7, 9), (8, 1)]),                                             # = and X across the tile edge
            (1, 0, [])]                                                                                 # no ops: never counted
    queries, pairs, spans, stride = [], [], [], 8
    cigar, n_cigar = np.zeros((len(plan), stride), np.uint32), np.zeros(len(plan), np.uint32)
    for p, (t, b0, ops) in enumerate(plan):
        q, j = "", b0
        for k, (op, n) in enumerate(ops):
            cigar[p, k] = (n << 4) | op
            if op == 7:
                q += targets[t][j:j + n]
            elif op == 8:
                q += "".join(BASES[(BASES.index(c) + 1 + p % 3) % 4] for c in targets[t][j:j + n])
            elif op == 1:
                q += "GAT"[:n]
            j += 0 if op == 1 else n
        n_cigar[p] = len(ops)
        queries.append(q or "A")
        pairs.append((p, t, 0))
        spans.append((0, len(q), b0, j) if ops else (0, 0, 0, 0))
    assert any(b0 < T < b0 + sum(n for op, n in ops if op != 1) for t, b0, ops in plan if t == 2)        # a row across the tile edge
    A, B = gpu_ctx.upload(queries), gpu_ctx.upload(targets)
    off = np.concatenate([[0], np.cumsum(lens)])
    got = []
    for scores in ([1] * len(plan), [(0, -5, 7)[p % 3] for p in range(len(plan))]):
        aln = np.array([(s, 0) + span for s, span in zip(scores, spans)], pkg.ffi.AFFINE_DTYPE)
        haps, heads = gpu_ctx.pileup_hap(A, B, pairs, aln, cigar, n_cigar)
        got.append((gpu_ctx.pileup(A, B, pairs, aln, cigar, n_cigar), gpu_ctx.pileup_ins(A, B, pairs, aln, cigar, n_cigar), haps, heads))
        want_hap = hap_ref.records(pairs, aln, cigar, n_cigar, queries, lens, need_score=False)
        for have, ref in zip(got[-1][0], pr.pileup(queries, lens, pairs, aln, cigar, n_cigar)):
            assert (pr.as_table(have) == ref).all()
        assert ins_ref.as_rows(got[-1][1]) == ins_ref.records(pairs, aln, cigar, n_cigar, queries, off, need_score=False)
        assert hap_ref.as_rows(haps) == want_hap[0] and hap_ref.as_heads(heads) == want_hap[1]
    assert len(got[0][1]) >= 3 and len(got[0][2]) >= 3 and all(h["n_cols"] > 0 for h in got[0][3])      # the lists are not empty
    flat = lambda g: (b"".join(t.tobytes() for t in g[0]), g[1].tobytes(), g[2].tobytes(), g[3].tobytes())
    assert flat(got[0]) == flat(got[1])


def raw_call(b, gpu_ctx, cigar, n_cigar=None):
    ffi = b["ffi"]
    rows = np.zeros(len(b["pairs"]), ffi.PAIR_DTYPE)
    for i, p in enumerate(b["pairs"]):
        rows[i] = (p[0], p[1], p[2], 0)
    off = np.zeros(len(b["lens"]) + 1, np.uint64)
    off[1:] = np.cumsum(b["lens"])
    out = np.full(int(off[-1]) * 8, 0xABABABAB, np.uint32)
    aln = np.ascontiguousarray(b["aln"])
    cigar = np.ascontiguousarray(cigar, np.uint32)
    n_cigar = np.ascontiguousarray(b["n_cigar"] if n_cigar is None else n_cigar, np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = ffi.lib().sp_pileup_batch(gpu_ctx._h, b["A"]._h, b["B"]._h, ptr(rows), len(rows), ptr(aln), ptr(cigar), cigar.shape[1], ptr(n_cigar), ptr(off), ptr(out))
    return rc, out


def test_bad_ops_are_an_argument_error_before_any_launch(batch, gpu_ctx):
    b, ffi = batch, batch["ffi"]
    p = int(np.argmax(b["n_cigar"]))
    longer = b["cigar"].copy()
    longer[p, 3] += 1 << 4                                                                              # one run one base longer
    rc, out = raw_call(b, gpu_ctx, longer)
    assert rc == ffi.SP_ERR_INVALID_ARG and (out == 0xABABABAB).all()                                   # nothing written
    assert "do not consume" in ffi.lib().sp_last_error(gpu_ctx._h).decode()
    # an insertion before the alignment's first target column: pair 0 is one run of '='; I D = consume the same bases of both sequences
    assert b["n_cigar"][0] == 1 and int(b["cigar"][0][0]) & 15 == 7 and int(b["cigar"][0][0]) >> 4 > 2
    first_i, nc = b["cigar"].copy(), b["n_cigar"].copy()
    first_i[0, :3] = [(1 << 4) | 1, (1 << 4) | 2, (((int(b["cigar"][0][0]) >> 4) - 1) << 4) | 7]
    nc[0] = 3
    rc, out = raw_call(b, gpu_ctx, first_i, nc)
    assert rc == ffi.SP_ERR_INVALID_ARG and (out == 0xABABABAB).all()
    assert "insertion before" in ffi.lib().sp_last_error(gpu_ctx._h).decode()
    rc, out = raw_call(b, gpu_ctx, b["cigar"])                                                          # and the untouched batch still runs
    assert rc == ffi.SP_OK and out.tobytes() == b"".join(t.tobytes() for t in b["got"])


def test_a_warm_call_allocates_nothing(batch, gpu_ctx):
    b = batch
    before = gpu_ctx.profile_get("pool:device")
    gpu_ctx.pileup(b["A"], b["B"], b["pairs"], b["aln"], b["cigar"], b["n_cigar"])
    assert gpu_ctx.profile_get("pool:device")[1:] == before[1:]

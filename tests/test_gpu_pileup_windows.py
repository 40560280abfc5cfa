"""sp_pileup_windows_batch (window_kernel, sp_pileup.hip) against tests/pileup_win_ref.py, count for count, on the hand-made op rows of tests/pileup_win_cases.py:
windows from b_start and to b_end and each shifted by one; 'X' on the first and on the last column of a window; a 'D' run entering and one leaving a window; an 'I' at
both outer junctions (still exact) and at the first and last interior junction (not); nested, identical and overlapping windows; one window per column of a 70-base
target; a target without windows, one without pairs, a pair with n_cigar 0; pairs of 65, 129, 299 and 601 ops (past a wave's 64 ops, and past the defects a wave
holds in one round); SP_WINDOW_CHUNK - 1, SP_WINDOW_CHUNK and SP_WINDOW_CHUNK + 1 windows on one target; the pairs shuffled."""
import numpy as np
import pytest

import pileup_win_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batch(pkg, gpu_ctx):
    ffi = pkg.ffi
    case = cases.build(ffi.SP_WINDOW_CHUNK)
    rng = np.random.default_rng(3)
    seq = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, n))
    A, B = gpu_ctx.upload([seq(n) for n in case["q_len"]]), gpu_ctx.upload([seq(n) for n in case["t_len"]])
    pairs, aln, cigar, n_cigar = cases.arrays(ffi, case)
    got = gpu_ctx.pileup_windows(A, B, pairs, aln, cigar, n_cigar, case["windows"])
    return dict(ffi=ffi, case=case, A=A, B=B, got=got, want=cases.want(case))


def rows_of(tab):
    return [(int(r["span"]), int(r["exact"]), int(r["partial"])) for r in tab]


def test_every_count_equals_the_reference(batch):
    b = batch
    assert len(b["got"]) == len(b["want"])
    for t, tab in enumerate(b["got"]):
        assert rows_of(tab) == b["want"][t], t
        assert (tab["reserved_"] == 0).all()
    sizes = [len(w) for w in b["case"]["windows"]]
    C = b["ffi"].SP_WINDOW_CHUNK
    assert C - 1 in sizes and C in sizes and C + 1 in sizes and 0 in sizes
    assert max(len(a[2]) for a in b["case"]["alns"] if a) > 2 * b["ffi"].SP_WINDOW_DEFECTS          # a pair decided in more than one round
    assert any(x < s for tab in b["want"] for s, x, p in tab) and any(p for tab in b["want"] for s, x, p in tab)


def test_pair_order_does_not_matter(batch, gpu_ctx):
    b = batch
    order = np.random.default_rng(11).permutation(len(b["case"]["pairs"]))
    pairs, aln, cigar, n_cigar = cases.arrays(b["ffi"], b["case"], order)
    again = gpu_ctx.pileup_windows(b["A"], b["B"], pairs, aln, cigar, n_cigar, b["case"]["windows"])
    assert [x.tobytes() for x in again] == [x.tobytes() for x in b["got"]]


def test_a_warm_call_allocates_nothing(batch, gpu_ctx):
    b = batch
    pairs, aln, cigar, n_cigar = cases.arrays(b["ffi"], b["case"])
    gpu_ctx.pileup_windows(b["A"], b["B"], pairs, aln, cigar, n_cigar, b["case"]["windows"])
    before = gpu_ctx.profile_get("pool:device")
    again = gpu_ctx.pileup_windows(b["A"], b["B"], pairs, aln, cigar, n_cigar, b["case"]["windows"])
    assert gpu_ctx.profile_get("pool:device")[1:] == before[1:]
    assert [x.tobytes() for x in again] == [x.tobytes() for x in b["got"]]


def test_bad_windows_are_refused_before_any_launch(pkg, batch, gpu_ctx):
    b, ffi = batch, batch["ffi"]
    pairs, aln, cigar, n_cigar = cases.arrays(ffi, b["case"])
    launches = lambda: gpu_ctx.profile_get("pileup_windows")[1]
    n0 = launches()
    n_t = len(b["case"]["t_len"])
    flat = [w for ws in b["case"]["windows"] for w in ws]
    woff = np.zeros(n_t + 1, np.uint64)
    woff[1:] = np.cumsum([len(w) for w in b["case"]["windows"]])
    bad_lists = []
    for bad in ((5, 5), (6, 5), (60, 71)):                                  # empty, reversed, beyond its target of 70 columns
        bad_lists.append(([bad] + flat[1:], woff))
    down = woff.copy()
    down[2] = down[1] - 1                                                   # a win_offset that does not ascend
    bad_lists.append((flat, down))
    up = woff.copy()
    up[0] = 1
    bad_lists.append((flat, up))
    for windows, off in bad_lists:
        with pytest.raises(pkg.StarphaseError) as e:
            gpu_ctx.pileup_windows(b["A"], b["B"], pairs, aln, cigar, n_cigar, windows, win_offset=off)
        assert e.value.code == ffi.SP_ERR_INVALID_ARG
    assert launches() == n0
    ok = gpu_ctx.pileup_windows(b["A"], b["B"], pairs, aln, cigar, n_cigar, flat, win_offset=woff)
    assert launches() == n0 + 1 and [x.tobytes() for x in ok] == [x.tobytes() for x in b["got"]]


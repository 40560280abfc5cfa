"""Designed inputs for window support, as hand-made op rows (no aligner involved): shared by the CPU self-check of tests/pileup_win_ref.py and by the GPU test of
sp_pileup_windows_batch.  build(chunk) -> dict(t_len, q_len, pairs, alns, windows): alns[i] = (b_start, a_start, ops) or None (n_cigar 0)."""
import numpy as np

import pileup_win_ref as ref


def random_ops(rng, room, n_ops):
    """n_ops random ops that consume at most `room` target bases; never an 'I' first, no two 'I' in a row"""
    ops, used, last = [], 0, None
    for k in range(n_ops):
        kinds = [ref.EQ, ref.X, ref.D] + ([ref.I] if k and last != ref.I else [])
        kinds = [c for c in kinds if c != last]
        code = kinds[int(rng.integers(0, len(kinds)))]
        n = int(rng.integers(1, 4))
        if code != ref.I:
            if used + n > room:
                break
            used += n
        ops.append(ref.op(code, n))
        last = code
    return ops


def build(chunk):
    rng = np.random.default_rng(2024)
    t_len, q_len, pairs, alns, windows = [], [], [], [], []

    def add(t, b_start, ops, a_start=0):
        q_len.append(a_start + (ref.spans(ops)[1] if ops else 10) + 3)
        pairs.append((len(q_len) - 1, t))
        alns.append((b_start, a_start, list(ops)) if ops else None)

    # ---- target 0: 70 columns, the designed edges.  The main pair covers [5, 69): X on column 25, D on 36..38, an insertion between columns 48 and 49
    t_len.append(70)
    main = ref.ops_of("20= 1X 10= 3D 10= 2I 20=")
    add(0, 5, main, a_start=2)
    add(0, 0, ref.ops_of("70="))
    add(0, 10, [])                                                          # n_cigar 0
    add(0, 3, ref.ops_of("1=" + " 1X 1=" * 32))                             # 65 ops: one past a wave's batch of 64
    w0 = [(j, j + 1) for j in range(70)]                                    # one window per column
    w0 += [(5, 69), (6, 69), (5, 68), (4, 69), (5, 70), (6, 68)]            # from b_start, to b_end, each shifted by one
    w0 += [(25, 30), (20, 26), (24, 27)]                                    # X on the first / the last column, inside
    w0 += [(30, 37), (38, 45), (36, 39), (33, 36), (39, 42)]                # a D run entering, leaving, filling, and the windows beside it
    w0 += [(49, 55), (40, 49), (48, 55), (40, 50), (48, 50), (49, 50), (48, 49)]   # I at the left / right outer junction (exact), at the first / last interior one (not)
    w0 += [(10, 60), (20, 50), (20, 50), (15, 55), (45, 65), (50, 69), (0, 70), (0, 5), (69, 70)]   # nested, identical, overlapping, outside the main pair
    windows.append(w0)
    # ---- target 1: 300 columns, a pair of 129 ops and one with more defects than a wave holds in one round
    t_len.append(300)
    add(1, 7, ref.ops_of("1=" + " 1X 1=" * 64))                             # 129 ops over 129 columns
    add(1, 0, ref.ops_of("1=" + " 1X 1=" * 149))                            # 299 ops, 149 defects
    add(1, 20, ref.ops_of("5=" + " 1D 2= 1I 2=" * 50))                      # 201 ops, 100 defects
    windows.append([(j, j + w) for w in (1, 2, 3, 7) for j in range(0, 300 - w, 11)] + [(0, 300), (7, 136), (8, 135)])
    # ---- target 2: windows but no pair; target 3: pairs but no windows
    t_len.append(50)
    windows.append([(0, 50), (10, 20)])
    t_len.append(60)
    add(3, 0, ref.ops_of("60="))
    windows.append([])
    # ---- targets 4, 5, 6: chunk - 1, chunk and chunk + 1 windows over random pairs
    for k, n_w in enumerate((chunk - 1, chunk, chunk + 1)):
        t = 4 + k
        t_len.append(240)
        for _ in range(9):
            b_start = int(rng.integers(0, 60))
            ops = random_ops(rng, 240 - b_start, int(rng.integers(3, 150)))
            add(t, b_start, ops, a_start=int(rng.integers(0, 4)))
        w = []
        for _ in range(n_w):
            s = int(rng.integers(0, 239))
            w.append((s, int(rng.integers(s + 1, min(240, s + 40) + 1))))
        windows.append(w)
    # ---- target 7: 700 columns, a pair with 600 ops and 300 defects (three rounds of the wave's defect buffer), beside a clean one
    t_len.append(700)
    add(7, 10, ref.ops_of("1=" + " 1X 1=" * 300))
    add(7, 0, ref.ops_of("700="))
    windows.append([(j, j + w) for w in (1, 2, 5) for j in range(0, 690, 13)] + [(10, 611), (0, 700)])
    return dict(t_len=t_len, q_len=q_len, pairs=pairs, alns=alns, windows=windows)


def want(case):
    return ref.window_support(case["pairs"], [None if a is None else (a[0], a[2]) for a in case["alns"]], case["windows"])


def arrays(ffi, case, order=None):
    """the arguments of Context.pileup_windows for the case: (pairs, aln, cigar, n_cigar); order: a permutation of the pairs"""
    idx = list(range(len(case["pairs"]))) if order is None else list(order)
    stride = max(len(a[2]) for a in case["alns"] if a is not None)
    aln = np.zeros(len(idx), ffi.AFFINE_DTYPE)
    cigar = np.zeros((len(idx), stride), np.uint32)
    n_cigar = np.zeros(len(idx), np.uint32)
    pairs = []
    for k, i in enumerate(idx):
        q, t = case["pairs"][i]
        pairs.append((q, t, 0, 0))
        a = case["alns"][i]
        if a is None:
            continue
        tl, ql = ref.spans(a[2])
        aln[k] = (1, 0, a[1], a[1] + ql, a[0], a[0] + tl)
        cigar[k, :len(a[2])] = a[2]
        n_cigar[k] = len(a[2])
    return pairs, aln, cigar, n_cigar

"""Window support without a device: the new entry points answer a call without a context as the entries beside them do (an error code, nothing written, never a CPU
fallback), the header and the binding agree on the geometry, and tests/pileup_win_ref.py -- the reference the GPU tests hold the kernel to -- agrees with its own
per-column brute force on every designed case.  No compute call is made here."""
import ctypes as C
import os
import re

import numpy as np

import pileup_win_cases as cases
import pileup_win_ref as ref


def test_the_new_entries_without_a_context_are_errors(pkg):
    ffi, db = pkg.ffi, pkg.database
    lib, dlib = ffi.lib(), db._lib()
    h = C.c_void_p()
    rc = lib.sp_ctx_create(0, None, C.byref(h))
    if rc == ffi.SP_OK:                                                     # a machine with a device: the handle is not used here
        lib.sp_ctx_destroy(h)
    else:
        assert rc == ffi.SP_ERR_NO_DEVICE and not h.value
    op = ffi.sp_affine_opts(1, 4, 6, 2, 26, 1, 1)
    rows = np.zeros(1, ffi.PAIR_DTYPE)
    off = np.zeros(4, np.uint64)
    win = np.zeros(2, ffi.WINDOW_DTYPE)
    win[0] = (0, 1)
    out = np.full(2, 0x5A, ffi.WINDOW_SUPPORT_DTYPE)
    ok = np.full(2, 0x5A, np.int32)
    before = out.tobytes() + ok.tobytes()
    ptr = ffi._ptr
    call = ffi.sp_cyp_call()
    pr = ffi.sp_cyp_problem()
    rv = ffi.sp_cyp_region_variants()
    old = lib.sp_align_pileup_band_batch(None, None, None, ptr(rows), 1, C.byref(op), 64, 256, ptr(off), None, None, None, None, None)
    got = [lib.sp_align_pileup_windows_batch(None, None, None, ptr(rows), 1, C.byref(op), 64, 256, ptr(off), None, None, None, None, None, ptr(off), ptr(win), ptr(out)),
           lib.sp_pileup_windows_batch(None, None, None, ptr(rows), 1, None, None, 0, None, ptr(off), ptr(off), ptr(win), ptr(out)),
           dlib.sp_cyp_variant_support(None, C.byref(pr), None, C.byref(call), None, 0, C.byref(rv), None, 0, 2, ptr(out), ptr(ok), None, None, 0, None),
           dlib.sp_cyp_variant_support_cohort(None, C.byref(pr), 1, None, C.byref(call), None, 0, C.byref(rv), None, ptr(off), 2, ptr(out), ptr(ok), None, None, 0, None)]
    assert got == [old] * 4 and old == ffi.SP_ERR_INVALID_ARG
    assert out.tobytes() + ok.tobytes() == before
    assert lib.sp_struct_size(b"sp_window") == ffi.WINDOW_DTYPE.itemsize == C.sizeof(ffi.sp_window) == 8
    assert lib.sp_struct_size(b"sp_window_support") == ffi.WINDOW_SUPPORT_DTYPE.itemsize == C.sizeof(ffi.sp_window_support) == 16


def test_the_header_and_the_binding_agree_on_the_geometry(pkg):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "starphase_hip.h")).read()
    for name in ("SP_WINDOW_CHUNK", "SP_WINDOW_WAVES", "SP_WINDOW_DEFECTS"):
        assert int(re.search(r"#define %s\s+(\d+)" % name, header).group(1)) == getattr(pkg.ffi, name)
    assert int(re.search(r"#define SP_CYP_VCF_FLANK\s+(\d+)", header).group(1)) == pkg.database.SP_CYP_VCF_FLANK == 2
    assert pkg.ffi.SP_WINDOW_CHUNK % 64 == 0 and pkg.ffi.SP_WINDOW_CHUNK <= 64 * pkg.ffi.SP_WINDOW_WAVES and pkg.ffi.SP_WINDOW_DEFECTS >= 128


def test_the_reference_agrees_with_its_brute_force_on_the_designed_cases(pkg):
    case = cases.build(pkg.ffi.SP_WINDOW_CHUNK)
    n = 0
    for (q, t), a in zip(case["pairs"], case["alns"]):
        if a is None:
            continue
        for s, e in case["windows"][t]:
            assert ref.window_of_pair(a[0], a[2], s, e) == ref.window_of_pair_brute(a[0], a[2], s, e), (t, a[0], s, e)
            n += 1
    assert n > 3000
    # the designed edges of target 0, spelled out: (span, exact, partial) of the main pair alone
    main = case["alns"][0]
    one = lambda s, e: ref.window_of_pair(main[0], main[2], s, e)
    assert one(5, 69) == (1, 0, 0) and one(4, 69) == (0, 0, 1) and one(5, 70) == (0, 0, 1) and one(0, 5) == (0, 0, 0) and one(69, 70) == (0, 0, 0)
    assert one(25, 30) == (1, 0, 0) and one(20, 26) == (1, 0, 0) and one(26, 30) == (1, 1, 0)
    assert one(30, 37) == (1, 0, 0) and one(38, 45) == (1, 0, 0) and one(33, 36) == (1, 1, 0) and one(39, 42) == (1, 1, 0)
    assert one(49, 55) == (1, 1, 0) and one(40, 49) == (1, 1, 0)            # the insertion at an outer junction, on either side: still exact
    assert one(48, 55) == (1, 0, 0) and one(40, 50) == (1, 0, 0)            # at the first / the last interior junction: not
    assert one(48, 49) == (1, 1, 0) and one(49, 50) == (1, 1, 0) and one(48, 50) == (1, 0, 0)
    want = cases.want(case)
    assert want[2] == [(0, 0, 0)] * 2 and want[3] == []
    for t, rows in enumerate(want):                                          # exact <= span, span + partial <= the aligned pairs of the target
        n_al = sum(1 for (q, tt), a in zip(case["pairs"], case["alns"]) if tt == t and a is not None)
        assert all(x <= s and s + p <= n_al for s, x, p in rows)

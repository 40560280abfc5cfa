"""The insertion-list entry points without a device: there is no context to run on (sp_ctx_create fails with SP_ERR_NO_DEVICE and hands out no handle), and every new
device entry answers a call without one as the entries beside it do -- an error code, nothing written, never a CPU fallback.  sp_support_ins_string is host code: a
record's string comes back from its key.  No compute call is made here."""
import ctypes as C

import numpy as np
import pytest

import pileup_ins_ref as ref


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
    ins = np.full(2, 0x5A, ffi.INS_DTYPE)
    before = ins.tobytes()
    n = C.c_uint64(77)
    ptr = ffi._ptr
    sm = ffi.sp_support_summary()
    call = ffi.sp_cyp_call()
    old = lib.sp_align_pileup_band_batch(None, None, None, ptr(rows), 1, C.byref(op), 64, 256, ptr(off), None, None, None, None, None)
    got = [lib.sp_align_pileup_ins_batch(None, None, None, ptr(rows), 1, C.byref(op), 64, 256, ptr(off), None, None, None, None, None, ptr(ins), 2, C.byref(n)),
           lib.sp_pileup_ins_batch(None, None, None, ptr(rows), 1, None, None, 0, None, ptr(off), ptr(ins), 2, C.byref(n)),
           lib.sp_hla_consensus_support_ins(None, None, 0, None, None, None, b"ACGT", b"", None, None, C.byref(sm), C.byref(sm), ptr(ins), 2, C.byref(n)),
           lib.sp_hla_consensus_support_cohort_ins(None, None, 1, None, 0, None, None, None, None, None, 0, None, ptr(off), None, 0, None, ptr(ins), 2, C.byref(n)),
           dlib.sp_cyp_consensus_support_ins(None, None, C.byref(call), None, 0, None, 0, ptr(off), None, 0, None, ptr(ins), 2, C.byref(n)),
           dlib.sp_cyp_consensus_support_cohort_ins(None, 1, None, C.byref(call), None, 0, None, ptr(off), ptr(off), None, 0, None, ptr(ins), 2, C.byref(n))]
    assert got == [old] * 6 and old == ffi.SP_ERR_INVALID_ARG
    assert ins.tobytes() == before and n.value == 77
    assert lib.sp_struct_size(b"sp_pileup_ins") == ffi.INS_DTYPE.itemsize == 56 and ffi.INS_DTYPE.itemsize % 8 == 0


@pytest.mark.parametrize("length", [1, 32, 33, 64])
def test_a_records_string_comes_back_from_its_key(pkg, length):
    ffi = pkg.ffi
    rng = np.random.default_rng(length)
    s = "".join("ACGT"[i] for i in rng.integers(0, 4, length))
    n, p0, p1, h = ref.key_of(s)
    rec = np.zeros(1, ffi.INS_DTYPE)
    rec[0] = (5, n, 1, p0, p1, h, 0, 0, 0, 0)
    assert ffi.support_ins_string(rec[0]) == s
    # the room it needs, and the answer when there is less
    need = C.c_uint64(0)
    small = C.create_string_buffer(length)
    assert ffi.lib().sp_support_ins_string(ffi._ptr(rec), None, 0, small, length, C.byref(need)) == ffi.SP_ERR_CAPACITY and need.value == length + 1
    # a longer record has no string without its query set
    rec[0]["len"] = 65
    assert ffi.lib().sp_support_ins_string(ffi._ptr(rec), None, 0, None, 0, C.byref(need)) == ffi.SP_ERR_INVALID_ARG


def test_the_header_and_the_binding_agree_on_the_runs_lds_holds(pkg):
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "starphase_hip.h")).read()
    assert int(re.search(r"#define SP_PILEUP_INS_LDS_RUNS\s+(\d+)", header).group(1)) == pkg.ffi.SP_PILEUP_INS_LDS_RUNS

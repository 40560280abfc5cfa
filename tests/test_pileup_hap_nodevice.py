"""The haplotype-list entry points without a device: every new device entry answers a call without a context as sp_align_pileup_band_batch does there -- an error
code, nothing written, never a CPU fallback.  sp_support_hap_string is host code: a record's calls come back as text.  No compute call is made here."""
import ctypes as C
import os
import re

import numpy as np

import pileup_hap_ref as ref


def test_the_new_entries_without_a_context_are_errors(pkg):
    ffi = pkg.ffi
    lib = ffi.lib()
    h = C.c_void_p()
    rc = lib.sp_ctx_create(0, None, C.byref(h))
    if rc == ffi.SP_OK:                                                     # a machine with a device: the handle is not used here
        lib.sp_ctx_destroy(h)
    else:
        assert rc == ffi.SP_ERR_NO_DEVICE and not h.value
    op = ffi.sp_affine_opts(1, 4, 6, 2, 26, 1, 1)
    rows = np.zeros(1, ffi.PAIR_DTYPE)
    off = np.zeros(4, np.uint64)
    haps = np.full(2, 0x5A, ffi.HAP_DTYPE)
    heads = np.full(2, 0x5A, ffi.HAP_HEAD_DTYPE)
    before = haps.tobytes() + heads.tobytes()
    n = C.c_uint64(77)
    ptr = ffi._ptr
    dlib = pkg.database._lib()
    sm = ffi.sp_support_summary()
    call = ffi.sp_cyp_call()
    old = lib.sp_align_pileup_band_batch(None, None, None, ptr(rows), 1, C.byref(op), 64, 256, ptr(off), None, None, None, None, None)
    got = [lib.sp_align_pileup_hap_batch(None, None, None, ptr(rows), 1, C.byref(op), 64, 256, ptr(off), None, None, None, None, None, None, 0, None,
                                         ptr(haps), 2, C.byref(n), ptr(heads)),
           lib.sp_pileup_hap_batch(None, None, None, ptr(rows), 1, None, None, 0, None, ptr(off), ptr(haps), 2, C.byref(n), ptr(heads)),
           lib.sp_hla_consensus_support_hap(None, None, 0, None, None, None, b"ACGT", b"", None, None, C.byref(sm), C.byref(sm), None, 0, None, ptr(haps), 2, C.byref(n), ptr(heads)),
           lib.sp_hla_consensus_support_cohort_hap(None, None, 1, None, 0, None, None, None, None, None, 0, None, ptr(off), None, 0, None, None, 0, None,
                                                   ptr(haps), 2, C.byref(n), ptr(heads)),
           dlib.sp_cyp_consensus_support_hap(None, None, C.byref(call), None, 0, None, 0, ptr(off), None, 0, None, None, 0, None, ptr(haps), 2, C.byref(n), ptr(heads)),
           dlib.sp_cyp_consensus_support_cohort_hap(None, 1, None, C.byref(call), None, 0, None, ptr(off), ptr(off), None, 0, None, None, 0, None, ptr(haps), 2, C.byref(n), ptr(heads))]
    assert got == [old] * 6 and old == ffi.SP_ERR_INVALID_ARG
    assert haps.tobytes() + heads.tobytes() == before and n.value == 77


def test_the_record_sizes(pkg):
    ffi = pkg.ffi
    assert ffi.lib().sp_struct_size(b"sp_support_hap") == ffi.HAP_DTYPE.itemsize == 56
    assert ffi.lib().sp_struct_size(b"sp_support_hap_head") == ffi.HAP_HEAD_DTYPE.itemsize == 24
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "starphase_hip.h")).read()
    assert int(re.search(r"#define SP_SUPPORT_HAP_COLS\s+(\d+)", header).group(1)) == ffi.SP_SUPPORT_HAP_COLS == ref.HAP_COLS == 64
    assert int(re.search(r"#define SP_SUPPORT_HAP_LDS_KEYS\s+(\d+)", header).group(1)) == ffi.SP_SUPPORT_HAP_LDS_KEYS


def record(ffi, calls, count=3, first=7, target=2):
    w = [0, 0, 0, 0]
    for k, c in enumerate(calls):
        w[k // 16] |= c << (4 * (k % 16))
    rec = np.zeros(1, ffi.HAP_DTYPE)
    rec[0] = (target, len(calls), count, first, 0, w)
    return rec


def test_a_records_calls_come_back_as_text(pkg):
    ffi = pkg.ffi
    rec = record(ffi, [1, 2, 3, 4, 5, 6, 0, 9, 8, 14])
    assert ffi.support_hap_string(rec[0]) == "=ACGT-?=+?+-+" == ref.text(ref.as_rows(rec)[0])
    assert ffi.support_hap_string(record(ffi, [])[0]) == ""
    # 64 columns: every word of the pattern, a '+' on the last call
    calls = [(k % 6) + 1 for k in range(63)] + [1 | 8]
    rec = record(ffi, calls)
    text = ffi.support_hap_string(rec[0])
    assert text == "".join("?=ACGT-"[c] for c in calls[:63]) + "=+" and len(text) == 65
    # the room it needs, and the answer when there is less; more columns than a pattern holds
    need = C.c_uint64(0)
    small = C.create_string_buffer(65)
    assert ffi.lib().sp_support_hap_string(ffi._ptr(rec), small, 65, C.byref(need)) == ffi.SP_ERR_CAPACITY and need.value == 66
    assert ffi.lib().sp_support_hap_string(ffi._ptr(rec), None, 0, C.byref(need)) == ffi.SP_ERR_CAPACITY and need.value == 66
    rec[0]["n_cols"] = 65
    assert ffi.lib().sp_support_hap_string(ffi._ptr(rec), small, 65, C.byref(need)) == ffi.SP_ERR_INVALID_ARG

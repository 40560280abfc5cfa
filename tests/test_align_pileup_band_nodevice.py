"""sp_align_pileup_band_batch without a device: there is no context to run on (sp_ctx_create fails with SP_ERR_NO_DEVICE and hands out no handle), and the new entry
answers a call without one exactly as sp_align_pileup_batch and the other batch calls do -- an error code, never a CPU fallback.  No compute call is made here."""
import ctypes as C

import numpy as np


def test_the_band_entry_without_a_context_is_the_error_of_the_other_batch_calls(pkg):
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
    off = np.zeros(2, np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    old = lib.sp_align_pileup_batch(None, None, None, ptr(rows), 1, C.byref(op), ptr(off), None, None, None, None)
    aln = np.full(6, 0x5A5A5A5A, np.uint32)
    used = np.full(1, 0xEFEFEFEF, np.uint32)
    for band, retry_band in ((64, 0), (256, 0), (64, 256)):
        new = lib.sp_align_pileup_band_batch(None, None, None, ptr(rows), 1, C.byref(op), band, retry_band, ptr(off), ptr(aln), None, None, None, ptr(used))
        assert new == old == ffi.SP_ERR_INVALID_ARG and new != ffi.SP_OK
    assert (aln == 0x5A5A5A5A).all() and (used == 0xEFEFEFEF).all()
    assert ffi.SP_ALIGN_PILEUP_WIDE_ROWS in (64, 128)


def test_the_header_and_the_binding_agree_on_the_rows_of_a_block(pkg):
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "starphase_hip.h")).read()
    assert int(re.search(r"#define SP_ALIGN_PILEUP_WIDE_ROWS\s+(\d+)", header).group(1)) == pkg.ffi.SP_ALIGN_PILEUP_WIDE_ROWS

"""The places where the two cohort support drivers (sp_hla_consensus_support_cohort_hap, sp_cyp_consensus_support_cohort_hap) differ, and the edges both share: a
consensus without any member, a slot without a target between two that have one, a list one record short, and the errors of either driver.  The expected values
are what the library returned before the two drivers were put on one support pass (csrc/sp_support.hip); the shared pass has to return the same.  Both entries
are called as the C header declares them, so that capacities and the caller's arrays are the test's own.  Fixtures: those of tests/test_gpu_consensus_support.py
and tests/test_gpu_cyp_support.py, edited as tests/test_gpu_support_hap.py edits them."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_consensus_support import calls  # noqa: F401  (the module's fixture)
from test_gpu_cyp_support import CONS_CAP, world  # noqa: F401
from test_gpu_support_hap import edited_cyp, edited_hla
from test_gpu_support_ins import gap_site

pytestmark = pytest.mark.gpu

INVALID_ARG, CAPACITY = 1, 6
FILL = 0xAB                                                               # what the caller's summaries and heads hold before a call
NAMES = ("consensus_support_map", "consensus_support_map_retry", "consensus_support_summary", "pileup", "align_pileup_map", "align_pileup_map_retry",
         "align_pileup_pile", "align_pileup_summary", "pileup_ins_collect", "pileup_ins_reduce", "support_hap")


def filled(n, dtype):
    return np.frombuffer(bytearray([FILL]) * (max(1, n) * np.dtype(dtype).itemsize), dtype)


def snapshot(ctx):
    return {n: ctx.profile_get(n)[1:] for n in NAMES}


def moved(ctx, before):
    """the profile names whose (launches, cells) moved since `before`, and by how much"""
    now = snapshot(ctx)
    return {n: (now[n][0] - before[n][0], now[n][1] - before[n][1]) for n in NAMES if now[n] != before[n]}


def outputs(ffi, n_slots, total):
    return dict(off=np.zeros(n_slots + 1, np.uint64), cols=np.zeros(max(1, total), ffi.PILEUP_DTYPE), sm=filled(n_slots, ffi.SUPPORT_DTYPE),
                ins=np.zeros(16384, ffi.INS_DTYPE), haps=np.zeros(16384, ffi.HAP_DTYPE), heads=filled(n_slots, ffi.HAP_HEAD_DTYPE), total=total)


def finish(ffi, ctx, o, rc, n_i, n_h):
    o.update(rc=rc, err=ffi.lib().sp_last_error(ctx._h).decode() if rc else "", n_ins=n_i.value, n_haps=n_h.value)
    return o


def hla_raw(pkg, c, genes, cons, rec=None, cols_cap=None, ins_cap=16384, hap_cap=16384):
    """sp_hla_consensus_support_cohort_hap on one sample: cons[k] = (consensus1, consensus2) of genes[k]"""
    ffi, db = pkg.ffi, c["db"]
    flat = [x for pair in cons for x in pair]
    cap = max(len(x) for x in flat) + 1
    buf = C.create_string_buffer(b"".join(x.encode().ljust(cap, b"\0") for x in flat), len(flat) * cap)
    g = np.ascontiguousarray(genes, np.uint32)
    rec = np.ascontiguousarray(c["rec"] if rec is None else rec)
    is1 = np.ascontiguousarray(c["is1"], np.uint8)
    o = outputs(ffi, len(flat), sum(len(x) for x in flat))
    n_i, n_h = C.c_uint64(0), C.c_uint64(0)
    rc = ffi.lib().sp_hla_consensus_support_cohort_hap(db.ctx._h, db._h, 1, None, len(genes), ffi._ptr(g), c["R"]._h, ffi._ptr(rec), ffi._ptr(is1), buf, cap, None, ffi._ptr(o["off"]),
                                                       ffi._ptr(o["cols"]), o["total"] if cols_cap is None else cols_cap, ffi._ptr(o["sm"]), ffi._ptr(o["ins"]), ins_cap, C.byref(n_i),
                                                       ffi._ptr(o["haps"]), hap_cap, C.byref(n_h), ffi._ptr(o["heads"]))
    return finish(ffi, db.ctx, o, rc, n_i, n_h)


def cyp_raw(pkg, ctx, ss, blocks=None, mappings=None, cols_cap=None, ins_cap=16384, hap_cap=16384):
    """sp_cyp_consensus_support_cohort_hap on the samples ss; blocks / mappings: other consensus blocks / mapping lists than the samples' own"""
    D, ffi = pkg.database, pkg.ffi
    n, M = len(ss), ffi.SP_CYP_MAXCONS
    blocks = [s["cons"] for s in ss] if blocks is None else blocks
    mappings = [s["mappings"] for s in ss] if mappings is None else mappings
    carr = (ffi.sp_cyp_call * n)()
    for i, s in enumerate(ss):
        C.memmove(C.byref(carr[i]), C.byref(s["call"]), C.sizeof(ffi.sp_cyp_call))
    block = C.create_string_buffer(b"".join(b.raw for b in blocks), n * M * CONS_CAP)
    flat = [m for ms in mappings for m in ms]
    moff = np.zeros(n + 1, np.uint64)
    moff[1:] = np.cumsum([len(ms) for ms in mappings])
    handles = (C.c_void_p * n)(*[s["R"]._h.value if isinstance(s["R"]._h, C.c_void_p) else s["R"]._h for s in ss])
    o = outputs(ffi, n * M, sum(len(D.cyp_consensus_of(blocks[i], CONS_CAP, h)) for i in range(n) for h in range(ss[i]["call"].n_consensus)))
    o.update(flat=flat, moff=moff)
    n_i, n_h = C.c_uint64(0), C.c_uint64(0)
    rc = D._lib().sp_cyp_consensus_support_cohort_hap(ctx._h, n, handles, carr, C.cast(block, C.c_void_p), CONS_CAP, D._mapping_array(flat), ffi._ptr(moff), ffi._ptr(o["off"]),
                                                      ffi._ptr(o["cols"]), o["total"] if cols_cap is None else cols_cap, ffi._ptr(o["sm"]), ffi._ptr(o["ins"]), ins_cap, C.byref(n_i),
                                                      ffi._ptr(o["haps"]), hap_cap, C.byref(n_h), ffi._ptr(o["heads"]))
    return finish(ffi, ctx, o, rc, n_i, n_h)


def summary(o, x):
    return tuple(int(v) for v in o["sm"][x])


def head(o, x):
    return tuple(int(v) for v in o["heads"][x])


def untouched(a):
    return a.tobytes() == bytes([FILL]) * a.nbytes


def zero(a):
    return not a.tobytes().strip(b"\0")


def blank(block, h):
    """the consensus block with consensus h empty"""
    raw = bytearray(block.raw)
    raw[h * CONS_CAP] = 0
    return C.create_string_buffer(bytes(raw), len(raw))


def changed(m, **fields):
    new = type(m).from_buffer_copy(m)
    for k, v in fields.items():
        setattr(new, k, v)
    return new


def same_tables(a, b):
    return a["off"].tobytes() == b["off"].tobytes() and a["cols"].tobytes() == b["cols"].tobytes() and a["sm"].tobytes() == b["sm"].tobytes()


def test_hla_a_consensus_without_members(calls, pkg, gpu_ctx):  # noqa: F811
    c = calls
    gene = c["genes"][1]
    pair = c["out"][1][1:]
    assert pair[0]
    rec = c["rec"].copy()
    rec["status"][rec["gene"] == gene] = 1                                 # no read of the gene is realigned
    before = snapshot(gpu_ctx)
    r = hla_raw(pkg, c, [gene], [pair], rec=rec)
    assert r["rc"] == 0 and moved(gpu_ctx, before) == {}                   # summarized on the host: no launch at all
    assert [summary(r, x) for x in range(2)] == [(0, 0, 0, len(s), 0, 0, 0, 0) for s in pair]
    assert zero(r["cols"]) and zero(r["heads"][:2]) and (r["n_ins"], r["n_haps"]) == (0, 0) and [int(x) for x in r["off"]] == [0, len(pair[0]), len(pair[0]) + len(pair[1])]
    # beside a gene that has its members the pass runs, once, and that gene's results are those of the call without the empty gene
    alone = hla_raw(pkg, c, c["genes"][:1], [c["out"][0][1:]])
    before = snapshot(gpu_ctx)
    both = hla_raw(pkg, c, c["genes"], [c["out"][0][1:], pair], rec=rec)
    delta = moved(gpu_ctx, before)
    assert alone["rc"] == both["rc"] == 0 and delta["consensus_support_map"][0] == 1 and delta["consensus_support_summary"][0] == 1 and delta["pileup"][0] == 1
    n0 = int(both["off"][2])
    assert both["cols"][:n0].tobytes() == alone["cols"][:n0].tobytes() and both["sm"][:2].tobytes() == alone["sm"][:2].tobytes() and summary(both, 0)[0] > 0
    assert [summary(both, x) for x in (2, 3)] == [(0, 0, 0, len(s), 0, 0, 0, 0) for s in pair] and zero(both["cols"][n0:])
    assert both["n_ins"] == alone["n_ins"] and both["ins"].tobytes() == alone["ins"].tobytes() and both["n_haps"] == alone["n_haps"]
    assert [head(both, x) for x in (2, 3)] == [(both["n_haps"], 0, 0, 0, 0)] * 2


# what a CYP2D6 support call over a sample without mapping records launches: the pass still runs -- the pileup and summary over the columns, both lists over no pair
def cyp_no_member_moves(total):
    return {"align_pileup_pile": (1, total), "align_pileup_summary": (1, total), "support_hap": (1, 0)}


def test_cyp_a_sample_without_mappings(world, pkg, gpu_ctx):  # noqa: F811
    s = world["samples"]["*1/*4"]
    H, M = s["call"].n_consensus, pkg.ffi.SP_CYP_MAXCONS
    before = snapshot(gpu_ctx)
    r = cyp_raw(pkg, gpu_ctx, [s], mappings=[[]])
    delta = moved(gpu_ctx, before)
    assert r["rc"] == 0 and delta == cyp_no_member_moves(r["total"])
    assert [summary(r, h) for h in range(H)] == [(0, 0, 0, len(t), 0, 0, 0, 0) for t in s["text"]] and zero(r["sm"][H:])
    assert zero(r["cols"]) and zero(r["heads"]) and (r["n_ins"], r["n_haps"]) == (0, 0)


def hla_planted(c, k, cons1, cut_len):
    """where the three bases deleted from consensus 1 of gene k come back as an insertion (gene-strand column), and as what"""
    p = gap_site(cons1, len(cons1) // 2)
    if c["fx"].gene_fwd[c["genes"][k]]:
        return p - 1, cons1[p:p + 3]
    return cut_len - p - 1, c["synth"].revcomp(cons1[p:p + 3])


def check_planted(pkg, o, col, want):
    """the first record of column `col` (in col_offset's space) is the planted string, and it makes the column contested"""
    mine = [r for r in o["ins"][:o["n_ins"]] if int(r["col"]) == col]
    assert mine and pkg.ffi.support_ins_string(mine[0]) == want and 2 * int(o["cols"][col]["ins"]) > int(o["cols"][col]["depth"]), (col, want)


def check_slots(o, live, n_slots):
    """heads, records and insertion columns of a call whose slots `live` have targets: an empty slot's head is zero but for first_record, which continues the running
    position; the records of a slot lie where its head says; every insertion column lies in a live slot's part of col_offset"""
    at = 0
    for x in range(n_slots):
        if x in live:
            assert head(o, x)[0] == at
            assert all(int(t) == x for t in o["haps"]["target"][at:at + head(o, x)[1]])
            at += head(o, x)[1]
        else:
            assert head(o, x) == (at, 0, 0, 0, 0), (x, head(o, x))
    assert at == o["n_haps"]
    spans = [(int(o["off"][x]), int(o["off"][x + 1])) for x in live]
    assert o["n_ins"] >= 1 and all(any(lo <= int(col) < hi for lo, hi in spans) for col in o["ins"]["col"][:o["n_ins"]])


def test_hla_a_slot_without_a_target_between_two(calls, pkg):  # noqa: F811
    c = calls
    cons = [(pair[0], "" if k == 0 else pair[1]) for k, pair in enumerate(edited_hla(c))]
    r = hla_raw(pkg, c, c["genes"], cons)
    assert r["rc"] == 0
    live = [x for x in range(4) if cons[x // 2][x % 2]]
    assert live[:2] == [0, 2] and head(r, 0)[1] >= 1 and head(r, 2)[1] >= 1
    check_slots(r, live, 4)
    assert head(r, 1) == (head(r, 0)[1], 0, 0, 0, 0) and summary(r, 1) == (0,) * 8
    for k in range(2):
        col, want = hla_planted(c, k, c["out"][k][1], len(cons[k][0]))
        check_planted(pkg, r, int(r["off"][2 * k]) + col, want)
    for rows in (r["ins"][:r["n_ins"]][r["ins"]["len"][:r["n_ins"]] > 0], r["haps"][:r["n_haps"]]):          # first_pair is a read of the slot's gene
        slot = [int(np.searchsorted(r["off"], int(x["col"]), "right")) - 1 for x in rows] if "col" in rows.dtype.names else [int(x["target"]) for x in rows]
        assert all(int(c["rec"][int(x["first_pair"])]["gene"]) == c["genes"][sl // 2] for x, sl in zip(rows, slot))


def test_cyp_a_slot_without_a_target_between_two(world, pkg, gpu_ctx):  # noqa: F811
    M = pkg.ffi.SP_CYP_MAXCONS
    ss = [world["samples"][n] for n in world["samples"]]
    blocks = [edited_cyp(s)[0] for s in ss]
    blocks[0] = blank(blocks[0], 1)
    r = cyp_raw(pkg, gpu_ctx, ss, blocks=blocks)
    assert r["rc"] == 0
    live = [i * M + h for i, s in enumerate(ss) for h in range(s["call"].n_consensus) if (i, h) != (0, 1)]
    assert head(r, 0)[1] >= 1 and head(r, M)[1] >= 1
    check_slots(r, live, 2 * M)
    assert head(r, 1) == (head(r, 0)[1], 0, 0, 0, 0) and summary(r, 1) == (0,) * 8 and r["off"][1] == r["off"][2]
    for i, s in enumerate(ss):
        p = gap_site(s["text"][0], len(s["text"][0]) // 2)
        check_planted(pkg, r, int(r["off"][i * M]) + p - 1, s["text"][0][p:p + 3])
    for x in r["haps"][:r["n_haps"]]:                                      # first_pair is a mapping record of the slot's sample and consensus
        i, h, k = int(x["target"]) // M, int(x["target"]) % M, int(x["first_pair"])
        assert int(r["moff"][i]) <= k < int(r["moff"][i + 1]) and r["flat"][k].consensus == h


def check_one_short(call, who):
    """a list one record short: SP_ERR_CAPACITY and the need, everything else complete, the other list included"""
    full = call()
    assert full["rc"] == 0 and full["n_ins"] >= 2 and full["n_haps"] >= 2
    ni, nh = full["n_ins"], full["n_haps"]
    a = call(ins_cap=ni - 1)
    assert a["rc"] == CAPACITY and a["n_ins"] == ni and a["err"] == f"{who}: {ni} insertion records, room for {ni - 1}"
    assert same_tables(a, full) and a["n_haps"] == nh and a["haps"].tobytes() == full["haps"].tobytes() and a["heads"].tobytes() == full["heads"].tobytes()
    b = call(hap_cap=nh - 1)
    assert b["rc"] == CAPACITY and b["n_haps"] == nh and b["err"] == f"{who}: {nh} haplotype records, room for {nh - 1}"
    assert same_tables(b, full) and b["n_ins"] == ni and b["ins"].tobytes() == full["ins"].tobytes()
    assert untouched(b["heads"]) and zero(b["haps"])                       # (nothing of a list that does not fit is written)


def test_hla_a_list_one_record_short(calls, pkg):  # noqa: F811
    c = calls
    check_one_short(lambda **kw: hla_raw(pkg, c, c["genes"], edited_hla(c), **kw), "consensus support")


def test_cyp_a_list_one_record_short(world, pkg, gpu_ctx):  # noqa: F811
    ss = [world["samples"][n] for n in world["samples"]]
    blocks = [edited_cyp(s)[0] for s in ss]
    check_one_short(lambda **kw: cyp_raw(pkg, gpu_ctx, ss, blocks=blocks, **kw), "align_pileup")              # (the pass names itself as the public entry does)


def test_hla_errors(calls, pkg):  # noqa: F811
    c = calls
    cons = [pair[1:] for pair in c["out"]]
    total = sum(len(x) for pair in cons for x in pair)
    r = hla_raw(pkg, c, c["genes"], cons, cols_cap=total - 1)
    assert (r["rc"], r["err"]) == (CAPACITY, f"consensus support: {total} columns, room for {total - 1}")
    assert untouched(r["sm"])                                              # the capacity is checked before the summaries are cleared
    member = [i for i in range(len(c["reads"])) if c["rec"][i]["status"] == 0 and c["rec"][i]["gene"] == c["genes"][0] and c["is1"][i]][0]
    rec = c["rec"].copy()
    rec["seg_end"][member] = len(c["reads"][member]) + 1
    r = hla_raw(pkg, c, c["genes"], cons, rec=rec)
    assert (r["rc"], r["err"]) == (INVALID_ARG, "consensus support: segment outside its read")
    r = hla_raw(pkg, c, [c["genes"][0]] * 2, [cons[0]] * 2)
    assert (r["rc"], r["err"]) == (INVALID_ARG, "consensus support: a gene is listed twice")


def test_cyp_errors(world, pkg, gpu_ctx):  # noqa: F811
    s = world["samples"]["*1/*4"]
    full = cyp_raw(pkg, gpu_ctx, [s])
    total = full["total"]
    assert full["rc"] == 0 and total == int(full["off"][-1])
    r = cyp_raw(pkg, gpu_ctx, [s], cols_cap=total - 1)
    assert (r["rc"], r["err"]) == (CAPACITY, f"cyp consensus support: {total} columns, room for {total - 1}")
    assert zero(r["sm"])                                                   # the summaries are cleared before the capacity is checked
    m0 = s["mappings"][0]
    for fields, text in ((dict(read_end=len(s["reads"][m0.read]) + 1), "cyp consensus support: segment outside its read"),
                         (dict(consensus=pkg.ffi.SP_CYP_MAXCONS), "cyp consensus support: mapping out of range"),
                         (dict(read=len(s["reads"])), "cyp consensus support: mapping out of range")):
        r = cyp_raw(pkg, gpu_ctx, [s], mappings=[[changed(m0, **fields)] + list(s["mappings"][1:])])
        assert (r["rc"], r["err"]) == (INVALID_ARG, text)

"""sp_anchor_batch, sp_anchor_batch_topk and sp_align_batch (HIP, through the C ABI) against the plain statement of the contract (tests/align_contract_ref.py) on the
designed cases of tests/align_contract_cases.py.  The oracle is not the judge here, and nothing compares the kernels with themselves: anchors, (ok, nm, a_end,
b_end) and the lengths come from the reference, the events are replayed as an alignment, and the untraced launch must report the row the traced one reports."""
import numpy as np
import pytest

import align_contract_cases as cases
import align_contract_ref as ref

pytestmark = pytest.mark.gpu

CELL_FAMILIES = sorted(cases.cell_families())
ANCHOR_FAMILIES = sorted(cases.anchor_families())
FIELDS = ("ok", "nm", "a_start", "a_end", "b_start", "b_end", "a_len", "b_len")


def _check_anchors(ctx, names, indexed, looked_up, want):
    """want[x] = the reference's four (diagonal, votes) of pair x; each family is its own pair of sets"""
    si, sl = ctx.upload(indexed), ctx.upload(looked_up)
    idx = np.arange(len(indexed), dtype=np.uint32)
    d4, v4 = ctx.anchor_batch_topk(si, sl, idx, idx, 4)
    d1, v1 = ctx.anchor_batch(si, sl, idx, idx)
    si.close(); sl.close()
    for x, w in enumerate(want):
        got = tuple((int(d), int(v)) for d, v in zip(d4[x], v4[x]))
        assert got == w, (names[x], got, w)
        assert (int(d1[x]), int(v1[x])) == w[0], (names[x], int(d1[x]), int(v1[x]), w[0])


@pytest.mark.parametrize("family", ANCHOR_FAMILIES)
def test_anchor_against_reference(gpu_ctx, family):
    cs = cases.anchor_families()[family]
    _check_anchors(gpu_ctx, [c.name for c in cs], [c.a for c in cs], [c.b for c in cs], [cases.ref_anchor(c.a, c.b, 4) for c in cs])


@pytest.mark.parametrize("family", CELL_FAMILIES)
def test_anchor_on_the_cell_cases(gpu_ctx, family):
    """the pairs of the cell families as anchor cases (B indexed, as the cell's callers do it)"""
    cs = cases.cell_families()[family]
    _check_anchors(gpu_ctx, [c.name for c in cs], [c.b for c in cs], [c.a for c in cs], [cases.ref_anchor(c.b, c.a, 4) for c in cs])


@pytest.mark.parametrize("family", CELL_FAMILIES)
def test_align_against_reference(gpu_ctx, family):
    cs = cases.cell_families()[family]
    sa, sb = gpu_ctx.upload([c.a for c in cs]), gpu_ctx.upload([c.b for c in cs])
    idx = np.arange(len(cs), dtype=np.uint32)
    diag = np.array([c.diag for c in cs], np.int32)
    cap = np.array([c.max_ed for c in cs], np.int32)
    traced, ev = gpu_ctx.align_batch(sa, sb, idx, idx, diag, cap, events=True)
    untraced = gpu_ctx.align_batch(sa, sb, idx, idx, diag, cap, events=False)
    sa.close(); sb.close()
    lost = 0
    for x, c in enumerate(cs):
        want = cases.ref_align(c)
        got = {f: int(traced[x][f]) for f in FIELDS}
        # a lost pair reports nothing: every field of the alignment is zero (the two lengths are the pair's, as in every row)
        exp = dict(ok=1, nm=want[0], a_end=want[1], b_end=want[2]) if want else dict(ok=0, nm=0, a_start=0, a_end=0, b_start=0, b_end=0)
        exp.update(a_len=len(c.a), b_len=len(c.b))
        assert {f: got[f] for f in exp} == exp, (c.name, got, want)
        assert {f: int(untraced[x][f]) for f in FIELDS} == got, (c.name, "untraced", untraced[x], got)
        if want:
            try:
                ref.replay(c.a, c.b, want[3], c.diag, (got["nm"], got["a_start"], got["a_end"], got["b_start"], got["b_end"]), ev[x, :got["nm"]])
            except AssertionError as e:
                raise AssertionError((c.name, "replay", got) + e.args) from None
        else:
            assert c.may_lose, c.name
            lost += 1
    print(f"{family}: {len(cs)} cases, {lost} lost")

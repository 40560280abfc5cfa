"""sp_cyp_variant_support and the VCF it feeds, through the step API on the CYP2D6 reads of tests/test_gpu_diplotype_files.py (the real variant table, ~120 reads):
the counts equal tests/pileup_win_ref.py run on the CIGARs Context.affine_align returns for the same pairs (the consensus onto the backbone on 256 diagonals for the
windows, every member onto its consensus on 64 diagonals for the counts), CR <= SR <= n_aligned everywhere, the GT columns follow the variant lists of
cyp2d6_alleles.json, and the table made beside the windows is the table of sp_cyp_consensus_support."""
import numpy as np
import pytest

import cyp_cases_real as cr
import pileup_win_ref as ref
from test_gpu_diplotype_files import Sample, fetch_order

pytestmark = pytest.mark.gpu
CONS_CAP = 65536


@pytest.fixture(scope="module")
def sample(pkg, tmp_path_factory):
    return Sample(tmp_path_factory.mktemp("sample"), pkg)


@pytest.fixture(scope="module")
def step(pkg, gpu_ctx, sample):
    D = pkg.database
    dbf, fasta = D.Database(sample.db), D.Fasta(sample.fasta)
    w_chrom, _ws, _we = dbf.cyp_window()
    cdb = dbf.cyp_db(gpu_ctx, fasta.fetch(w_chrom, sample.locus.start, sample.locus.start + len(sample.locus.sequence)), sample.locus.start)
    cfg, _gd = cr.load_db()
    keys = ("CYP2D6", "CYP2D7", "REP6", "REP7")
    s5 = cfg["cyp2d6_star5_del"]
    lo = min(min(cfg["cyp_coordinates"][k]["start"] for k in keys), s5["start"] - 500)
    hi = max(max(cfg["cyp_coordinates"][k]["end"] for k in keys), s5["end"] + 3000)
    reads = [r[2] for r in sorted(fetch_order(sample, [("chr22", lo, hi)], D), key=lambda x: x[1])]
    R = gpu_ctx.upload(reads)
    pr, call, cons, rv, mappings = D.cyp_call_with_variants(cdb, R, CONS_CAP)
    assert call.status == 0 and len(mappings) > 0
    sup, ok, (cols, sums) = D.cyp_variant_support(gpu_ctx, pr, R, call, cons, CONS_CAP, rv, mappings, table=True)
    consensus = [D.cyp_consensus_of(cons, CONS_CAP, h) for h in range(call.n_consensus)]
    return dict(D=D, cdb=cdb, pr=pr, reads=reads, R=R, call=call, cons=cons, rv=rv, mappings=mappings, sup=sup, ok=ok, cols=cols, sums=sums, consensus=consensus)


def test_the_counts_equal_the_reference_on_the_aligners_cigars(pkg, gpu_ctx, step):
    s, D = step, step["D"]
    H, NV = s["call"].n_consensus, int(s["pr"].n_variants)
    typed = [h for h in range(H) if s["rv"].has_variants[h] == 1]
    assert typed and NV == 393
    vs = s["cdb"].variants()
    import ctypes as C
    bb_start = vs[0][0] - int(C.cast(s["pr"].var_pos, C.POINTER(C.c_int32))[0])
    backbone = s["pr"].backbone[:s["pr"].backbone_len].decode()
    var_pos = [v[0] - bb_start for v in vs]
    ref_len = [len(v[1]) for v in vs]
    # ---- the windows: every typed consensus onto the backbone, one anchor for the diagonal, 256 diagonals
    T, BB = gpu_ctx.upload(s["consensus"]), gpu_ctx.upload([backbone])
    diag, votes = gpu_ctx.anchor_batch(T, BB, typed, [0] * len(typed))
    assert (votes > 0).all()
    aln, cigar, n_cigar = gpu_ctx.affine_align(T, BB, [(h, 0, int(d), 0) for h, d in zip(typed, diag)], a=1, band=256, cigar_stride=4096)
    windows = [[] for _ in range(H)]
    where = [[] for _ in range(H)]
    for k, h in enumerate(typed):
        assert 0 < int(n_cigar[k]) <= 4096
        ops = [int(w) for w in cigar[k, :int(n_cigar[k])]]
        got = D.cyp_variant_windows(aln[k], ops, var_pos, ref_len)
        want = [ref.lift(int(aln[k]["b_start"]), int(aln[k]["a_start"]), ops, p, n, D.SP_CYP_VCF_FLANK) for p, n in zip(var_pos, ref_len)]
        assert got == want
        for v, w in enumerate(got):
            assert bool(s["ok"][h, v]) == (w is not None)
            if w is not None:
                windows[h].append(w)
                where[h].append(v)
        assert len(windows[h]) > NV // 2
    untyped = [h for h in range(H) if h not in typed]
    assert not s["ok"][untyped].any() and not s["ok"][H:].any()
    # ---- the members: every mapping record onto its consensus, 64 diagonals, no second try
    segs = [s["reads"][m.read][m.read_start:m.read_end] for m in s["mappings"]]
    Q = gpu_ctx.upload(segs)
    m_t = [int(m.consensus) for m in s["mappings"]]
    diag, votes = gpu_ctx.anchor_batch(T, Q, m_t, list(range(len(segs))))
    pairs = [(i, m_t[i], -int(diag[i]) if votes[i] > 0 else 0, 0 if votes[i] > 0 else -1) for i in range(len(segs))]
    aln, cigar, n_cigar = gpu_ctx.affine_align(Q, T, pairs, a=1, band=64, cigar_stride=4096)
    alns = [(int(aln[i]["b_start"]), [int(w) for w in cigar[i, :int(n_cigar[i])]]) if int(n_cigar[i]) and int(aln[i]["score"]) > 0 else None for i in range(len(pairs))]
    want = ref.window_support([(p[0], p[1]) for p in pairs], alns, windows)
    n_inexact = 0
    for h in typed:
        n_aligned = s["sums"][h]["n_aligned"]
        assert n_aligned == sum(1 for i, a in enumerate(alns) if a is not None and m_t[i] == h)
        for (span, exact, partial), v in zip(want[h], where[h]):
            r = s["sup"][h, v]
            assert (int(r["span"]), int(r["exact"]), int(r["partial"])) == (span, exact, partial), (h, v)
            assert exact <= span <= n_aligned
            n_inexact += span - exact
        assert max(int(s["sup"][h, v]["span"]) for v in where[h]) >= 3
    assert n_inexact > 0                                                    # (HiFi errors: some spanning read disagrees somewhere)
    assert not s["sup"][~s["ok"].astype(bool)].view(np.uint32).any()        # no window: zero counts
    # ---- the table made beside the windows is the table of the call without them
    cols, sums = D.cyp_consensus_support(gpu_ctx, s["R"], s["call"], s["cons"], CONS_CAP, s["mappings"])
    assert sums == s["sums"] and [c.tobytes() for c in cols] == [c.tobytes() for c in s["cols"]]
    # ... ONE member pass serves both: the call with the table launches the map kernel once, as the call without it does
    maps = lambda: gpu_ctx.profile_get("align_pileup_map")[1]
    n0 = maps()
    D.cyp_variant_support(gpu_ctx, s["pr"], s["R"], s["call"], s["cons"], CONS_CAP, s["rv"], s["mappings"], table=True)
    assert maps() == n0 + 1
    # ... and without the table the counts are the same
    sup2, ok2 = D.cyp_variant_support(gpu_ctx, s["pr"], s["R"], s["call"], s["cons"], CONS_CAP, s["rv"], s["mappings"])
    assert sup2.tobytes() == s["sup"].tobytes() and ok2.tobytes() == s["ok"].tobytes()


def test_the_vcf_follows_the_variant_lists_of_cyp2d6_alleles_json(pkg, step):
    import ctypes as C
    import json
    s, D = step, step["D"]
    need = C.c_uint64(0)
    text = C.create_string_buffer(1 << 22)
    assert pkg.ffi.lib().sp_cyp_alleles_json(C.byref(s["pr"]), C.byref(s["call"]), C.byref(s["rv"]), text, len(text), C.byref(need)) == 0
    lists = json.loads(text.value.decode())["alleles"]
    codes = {n: k for k, n in enumerate(["Unknown", "Match", "Unexpected", "Missing", "AmbiguousUnexpected", "AmbiguousMissing", "UnknownUnexpected", "UnknownMissing"])}
    vcf = D.cyp_alleles_vcf(s["cdb"], s["call"], s["rv"], support=s["sup"], support_valid=s["ok"], file_date="20250102", command="x")
    lines = vcf.splitlines()
    head = [l for l in lines if l.startswith("#CHROM")][0].split("\t")
    names = head[9:]
    assert names == sorted(lists, key=lambda k: int(k.split("_", 1)[0])) and names
    records = {l.split("\t")[2]: l.split("\t") for l in lines if not l.startswith("#")}
    listed = {e["label"] for k in names for e in lists[k]}
    assert set(records) == listed
    for k, name in enumerate(names):
        h = int(name.split("_", 1)[0])
        state = {e["label"]: codes[e["variant_state"]] for e in lists[name]}
        for label, row in records.items():
            gt, sr, cr_ = row[9 + k].split(":")
            assert gt == ref.gt_of(state.get(label, 255))
            v = s["cdb"].index_label(label)
            if s["ok"][h, v]:
                assert (int(sr), int(cr_)) == (int(s["sup"][h, v]["span"]), int(s["sup"][h, v]["exact"])) and int(cr_) <= int(sr) <= s["sums"][h]["n_aligned"]
            else:
                assert (sr, cr_) == (".", ".")
    assert any(row[9].startswith("1:") for row in records.values())
    plain = D.cyp_alleles_vcf(s["cdb"], s["call"], s["rv"], file_date="20250102", command="x")
    assert [l.split("\t")[:9] + [c.split(":")[0] for c in l.split("\t")[9:]] for l in lines if not l.startswith("##")][1:] == \
           [l.split("\t")[:8] + ["GT:SR:CR"] + l.split("\t")[9:] for l in plain.splitlines() if not l.startswith("#")]

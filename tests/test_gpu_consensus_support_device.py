"""sp_hla_consensus_support on the device-resident pass (sp_align_pileup_band_batch's 64 diagonals with a second try on 256): a warm call allocates nothing, and the
alignments come from the map launch -- not from sp_affine_align_batch, whose direction rows are allocated and freed by every call.  (What the call returns is held
byte for byte by tests/test_gpu_consensus_support.py.)  The gene call is the one that file builds: a forward-strand and a reverse-strand gene of the synthetic database."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def calls(pkg, gpu_ctx):
    from pb_starphase_amd import synth
    fx = synth.HlaFixture(max_alleles_per_gene=40, seed=7)
    db = fx.make_db(pkg, gpu_ctx)
    rng = np.random.default_rng(11)
    fwd = [g for g in range(len(fx.genes)) if fx.gene_fwd[g] and fx.full_length_alleles(g)][0]
    rev = [g for g in range(len(fx.genes)) if not fx.gene_fwd[g] and fx.full_length_alleles(g)][0]
    reads = []
    for g, n in ((fwd, 9), (rev, 14)):
        a = fx.full_length_alleles(g)[0]
        hap, s = fx.haplotype(g, a)
        reads += synth.simulate_reads(rng, hap, s, len(fx.dna[a]), n, mean_len=6000, sd_len=800)
    R = gpu_ctx.upload(reads)
    rec = db.realign_reads(R)
    genes = [fwd, rev]
    out, is1 = db.diplotype_genes(genes, R, rec)
    yield dict(fx=fx, db=db, genes=genes, reads=reads, R=R, rec=rec, out=out, is1=is1, synth=synth)
    R.close()
    db.close()


def voted_members(c, gpu_ctx, gene, cons1, cons2):
    """the members of the call that sp_anchor_batch gives a vote: the pairs the support pass attempts"""
    synth, fx, rec = c["synth"], c["fx"], c["rec"]
    strand = (lambda s: s) if fx.gene_fwd[gene] else synth.revcomp
    targets = [strand(x) for x in (cons1, cons2)]
    queries, side = [], []
    for r in np.flatnonzero((rec["status"] == 0) & (rec["gene"] == gene)):
        k = 0 if c["is1"][r] else 1
        if targets[k]:
            queries.append(strand(c["reads"][r][int(rec[r]["seg_start"]):int(rec[r]["seg_end"])]))
            side.append(k)
    live = [k for k in range(2) if targets[k]]
    T, Q = gpu_ctx.upload([targets[k] for k in live]), gpu_ctx.upload(queries)
    diag, votes = gpu_ctx.anchor_batch(T, Q, [live.index(k) for k in side], list(range(len(queries))))
    T.close()
    Q.close()
    return int((np.asarray(votes) > 0).sum()), len(queries)


def test_a_warm_support_call_allocates_nothing_and_runs_the_map_launch(calls, gpu_ctx):
    c = calls
    for k, gene in enumerate(c["genes"]):
        call, cons1, cons2 = c["out"][k]
        assert call.status == 0 and cons1
        n_voted, n_members = voted_members(c, gpu_ctx, gene, cons1, cons2)
        assert 0 < n_voted <= n_members
        first = c["db"].consensus_support(gene, c["R"], c["rec"], c["is1"], cons1, cons2)
        pool = gpu_ctx.profile_get("pool:device")
        maps, rows = gpu_ctx.profile_get("consensus_support_map"), gpu_ctx.profile_get("affine_align")
        again = c["db"].consensus_support(gene, c["R"], c["rec"], c["is1"], cons1, cons2)
        assert gpu_ctx.profile_get("pool:device")[1:] == pool[1:]
        for side in range(2):
            assert again[side][0].tobytes() == first[side][0].tobytes() and again[side][1] == first[side][1]
        # the context's profile has no name for sp_affine_align_batch's direction rows (they are the call's own allocation): the call is held to its launches instead --
        # one map launch over the voted members, one second try, and no launch of the traceback kernel that needs those rows
        now = gpu_ctx.profile_get("consensus_support_map")
        assert now[1] == maps[1] + 1 and now[2] == maps[2] + n_voted
        assert gpu_ctx.profile_get("consensus_support_map_retry")[1] >= 2
        assert gpu_ctx.profile_get("affine_align")[1:] == rows[1:]
        assert sum(s[1]["n_aligned"] for s in again) <= n_voted and sum(s[1]["n_members"] for s in again) == n_members

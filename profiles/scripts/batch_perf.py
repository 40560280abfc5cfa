"""sp_starphase_call_batch against single sp_starphase_call runs on one handle: eight simulated fixture samples
(tests/test_gpu_diplotype_files.py's Sample: 95 HLA-A/-B reads, 120 CYP2D6 reads, two variant genes each), repeated to N samples.
usage: batch_perf.py OUT.json [--only-batch]   (--only-batch: no single calls in the process, for a kernel trace of batches alone)"""
import json
import os
import pathlib
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
from test_gpu_diplotype_files import Sample  # noqa: E402

only_batch = "--only-batch" in sys.argv
tmp = pathlib.Path(tempfile.mkdtemp())
samples = []
for k in range(8):
    (tmp / f"s{k}").mkdir()
    samples.append(Sample(tmp / f"s{k}", pkg, seed=41 + 17 * k))
inputs = lambda n: [dict(bams=samples[k % 8].bams, vcf=samples[k % 8].vcf) for k in range(n)]
out = {}
t0 = time.time()
h = pkg.database.Starphase(samples[0].db, samples[0].fasta)
out["create_ms"] = (time.time() - t0) * 1000
if not only_batch:
    # the first call of a handle builds the K1 seed index and warms the pools; the calls after it are the steady state
    calls = []
    for kw in inputs(16):
        h.call(**kw)
        calls.append(h.timing())
    out["single_first_call"] = calls[0]
    out["single_steady_call_ms_median"] = statistics.median(c["call_ms"] for c in calls[1:])
else:
    h.call_batch(inputs(8))
for n in ((32,) if only_batch else (32, 64)):
    if not only_batch:
        t0 = time.time()
        single = [h.call(**kw).json() for kw in inputs(n)]
        out[f"single_{n}_s"] = time.time() - t0
    for mg, th in ((None, None), (16, None), (64, 8)):
        t0 = time.time()
        got = h.call_batch(inputs(n), max_group=mg, threads=th)
        out[f"batch_{n}_group{mg or 64}_threads{th or 'default'}_s"] = time.time() - t0
        out[f"batch_{n}_group{mg or 64}_threads{th or 'default'}_timing"] = h.batch_timing()
        if not only_batch:
            assert [g.json() for g in got] == single
h.close()
json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out))

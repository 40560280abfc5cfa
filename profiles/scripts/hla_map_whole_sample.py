"""Whole-sample timing for the hla_debug.json mappings switch: batch_perf.py's steady single call and its 32-sample batch on ONE library.
usage: hla_map_whole_sample.py ROOT MODE   ROOT = a checkout with its library built (this one, or the parent commit's worktree);
MODE = plain (no debug folder: the comparison against the parent) | debug_off | debug_on (debug folders, the switch off / on: the added milliseconds).
Run it once per (ROOT, MODE) in a process of its own, alternating the two libraries, and take medians over the runs."""
import json, os, pathlib, statistics, sys, tempfile, time
HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT, MODE = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge
pkg = ge.load_package()
from test_gpu_diplotype_files import Sample
tmp = pathlib.Path(tempfile.mkdtemp())
samples = []
for k in range(8):
    (tmp / f"s{k}").mkdir(); samples.append(Sample(tmp / f"s{k}", pkg, seed=41 + 17 * k))
inputs = lambda n: [dict(bams=samples[k % 8].bams, vcf=samples[k % 8].vcf) for k in range(n)]
dbg = MODE != "plain"
kw = dict(debug_folder=str(tmp / "dbg1")) if dbg else {}
if dbg:
    (tmp / "dbg1").mkdir()
h = pkg.database.Starphase(samples[0].db, samples[0].fasta, **kw)
if MODE == "debug_on":
    h.set_hla_debug_mappings(True)
calls = []
for x in inputs(12):
    h.call(**x); calls.append(h.timing()["call_ms"])
h.close()
h = pkg.database.Starphase(samples[0].db, samples[0].fasta)
if MODE == "debug_on":
    h.set_hla_debug_mappings(True)
h.call_batch(inputs(8))
batch = []
for rep in range(3):
    folders = None
    if dbg:
        folders = [str(tmp / f"b{rep}_{i}") for i in range(32)]
        for f in folders:
            os.makedirs(f)
    t0 = time.time(); h.call_batch(inputs(32), debug_folders=folders); batch.append((time.time() - t0) * 1e3)
h.close()
print(json.dumps({"root": os.path.relpath(ROOT, HERE), "mode": MODE, "single_steady_call_ms_median": statistics.median(calls[1:]), "single_steady_call_ms": [round(c, 2) for c in calls[1:]],
                  "batch_32_ms_median": statistics.median(batch), "batch_32_ms": [round(b, 1) for b in batch]}))

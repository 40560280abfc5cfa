"""bench.py --dump-outputs on the host: structured records become one float64 column per field, strings byte rows, and outputs above the size limit
keep the same fixed, seeded share of their rows in every run"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_bench():
    """bench.py as a module, without the hardware-queue setting its import makes for the benchmark's own process"""
    had = os.environ.get("GPU_MAX_HW_QUEUES")
    import bench
    if had is None:
        os.environ.pop("GPU_MAX_HW_QUEUES", None)
    return bench


def test_dump_outputs_float_arrays_under_the_limit(tmp_path):
    bench = load_bench()
    rec = np.zeros(3, [("sample", np.int32), ("gene", np.int32), ("allele1", np.int32)])
    rec["allele1"] = [5, -1, 7]
    bench.dump_outputs(str(tmp_path / "a"), {"records": rec, "flags": np.array([True, False]), "text": bench._text_rows(["AC", "G"])})
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert got["records"].dtype == np.float64 and got["records"].tolist() == [[0, 0, 5], [0, 0, -1], [0, 0, 7]]
    assert got["flags"].dtype == np.float64 and got["flags"].tolist() == [1, 0]
    assert got["text"].dtype == np.float32 and got["text"].tolist() == [[65, 67], [71, 0]]
    big = {"x": np.arange(2 * bench.DUMP_LIMIT // 8, dtype=np.float64).reshape(-1, 4)}
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), big)
    x, y = np.load(tmp_path / "b" / "x.npy"), np.load(tmp_path / "c" / "x.npy")
    assert os.path.getsize(tmp_path / "b" / "x.npy") < 64_000_000 and len(x) > 0 and np.array_equal(x, y)
    assert (np.diff(x[:, 0]) > 0).all()                               # (rows in their original order)

"""hla_ties.json on hand-made class rows (host only: no device is touched): sp_hla_ties_json's layout, the 256-name cap and "more", a consensus whose scan has no
winner, a call without a typed allele (null), database order of the names, gene order, omitted genes."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("distinct", "score_only", "equal", "beats_winner", "winner")


def side(typed, winner, scan, cls, names, counts=None):
    cls = np.array(cls, np.uint8)
    return (typed, winner, scan, cls, np.bincount(cls, minlength=5) if counts is None else counts, names)


def test_layout_cap_and_nulls(pkg):
    ffi = pkg.ffi
    # 600 alleles in database order: 300 equal (beyond the cap), 2 score_only, 1 beats_winner, the winner, the rest distinct
    cls = [0] * 600
    for k in range(100, 400):
        cls[k] = 2
    cls[5], cls[450], cls[7], cls[50] = 1, 1, 3, 4
    names = ["HLA-A*%02d:%02d" % (k // 60 + 1, k % 60 + 1) for k in range(600)]
    a1 = side("HLA-A*01:51", "HLA-A*01:51", 1, cls, names)
    a2 = side(None, "HLA-A*01:03", 0, [2, 0, 4, 2], names[:4])                                     # a call without a typed allele: null
    b1 = side("HLA-B*07:02", None, 1, [0, 0, 0], ["HLA-B*07:02", "HLA-B*08:01", "HLA-B*15:01"], counts=[0, 0, 0, 0, 0])     # the scan has no winner: classes and counts 0
    entries = [("HLA-B", [b1, None]), ("HLA-DRB5", [None, None]), ("HLA-A", [a1, a2])]
    text = ffi.hla_ties_json(entries)
    doc = json.loads(text)
    assert text == json.dumps(doc, indent=2)                                                    # two-space layout, nothing that a JSON writer would put differently
    assert list(doc) == ["HLA-A", "HLA-B"]                                                       # gene order; a gene with neither consensus is omitted
    assert list(doc["HLA-A"]) == ["consensus1", "consensus2"] and list(doc["HLA-B"]) == ["consensus1"]
    r = doc["HLA-A"]["consensus1"]
    assert list(r) == ["typed_allele", "winner", "scan", "n_alleles", "counts", "equal", "score_only", "beats_winner"]
    assert (r["typed_allele"], r["winner"], r["scan"], r["n_alleles"]) == ("HLA-A*01:51", "HLA-A*01:51", "mm2", 600)
    assert r["counts"] == dict(distinct=296, score_only=2, equal=300, beats_winner=1, winner=1) and list(r["counts"]) == list(CLASSES)
    assert r["equal"] == {"names": names[100:356], "more": 44}                                    # the first 256 in database order, then how many were left out
    assert r["score_only"] == {"names": [names[5], names[450]]} and r["beats_winner"] == {"names": [names[7]]}
    r = doc["HLA-A"]["consensus2"]
    assert r["typed_allele"] is None and r["scan"] == "unit_cost" and r["equal"] == {"names": [names[0], names[3]]} and r["score_only"] == {"names": []}
    r = doc["HLA-B"]["consensus1"]
    assert r["winner"] is None and r["typed_allele"] == "HLA-B*07:02" and r["n_alleles"] == 3 and set(r["counts"].values()) == {0}
    assert all(r[k] == {"names": []} for k in ("equal", "score_only", "beats_winner"))
    # exactly 256 of a class: no "more"
    exact = side("x", "x", 1, [4] + [2] * 256, ["w"] + ["n%d" % k for k in range(256)])
    r = json.loads(ffi.hla_ties_json([("HLA-C", [exact, None])]))["HLA-C"]["consensus1"]
    assert len(r["equal"]["names"]) == 256 and "more" not in r["equal"]
    assert ffi.hla_ties_json([]) == "{}"


def test_refusals_and_the_buffer_protocol(pkg):
    ffi = pkg.ffi
    ok = side("x", "x", 1, [4, 2], ["a", "b"])
    with pytest.raises(pkg.StarphaseError):
        ffi.hla_ties_json([("HLA-A", [side("x", "x", 1, [4, 5], ["a", "b"], counts=[0] * 5), None])])       # no such class
    with pytest.raises(pkg.StarphaseError):
        ffi.hla_ties_json([("HLA-A", [side("x", "x", 2, [4, 2], ["a", "b"]), None])])                        # no such scan
    with pytest.raises(pkg.StarphaseError):
        ffi.hla_ties_json([("HLA-A", [ok, None]), ("HLA-A", [ok, None])])                                    # a gene given twice
    arr = (ffi.sp_hla_ties_entry * 1)()
    arr[0].gene = b"HLA-A"
    small, need = C.create_string_buffer(8), C.c_uint64(0)
    assert ffi.lib().sp_hla_ties_json(arr, 1, small, 8, C.byref(need)) == ffi.SP_OK and small.value == b"{}" and need.value == 3
    assert ffi.lib().sp_hla_ties_json(arr, 1, small, 2, C.byref(need)) == ffi.SP_ERR_CAPACITY and need.value == 3


def test_new_symbols_in_header_rust_block_and_binding(pkg):
    import inspect
    header = open(os.path.join(ROOT, "include", "starphase_hip.h")).read()
    rs = open(os.path.join(ROOT, "include", "starphase_hip.rs")).read()
    src = inspect.getsource(pkg.ffi) + inspect.getsource(pkg.database)
    L = pkg.ffi.lib()
    for name in ("sp_hla_map_consensus_ex", "sp_hla_map_consensus_batch_ex", "sp_hla_map_type_consensus_ex", "sp_hla_map_ties", "sp_hla_ties_json", "sp_starphase_set_hla_ties"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert "pub fn %s(" % name in rs, name
        assert '"%s"' % name in src, name
        assert hasattr(L, name), name
    assert L.sp_struct_size(b"sp_hla_ties_entry") == C.sizeof(pkg.ffi.sp_hla_ties_entry)
    assert int(re.search(r"#define SP_HLA_MAP_TIES\s+(\d+)", header).group(1)) == pkg.ffi.SP_HLA_MAP_TIES
    assert int(re.search(r"#define SP_HLA_TIES_MAX_NAMES\s+(\d+)", header).group(1)) == pkg.ffi.SP_HLA_TIES_MAX_NAMES
    for sub in ("diplotype", "diplotype-batch"):
        import subprocess
        assert "--debug-hla-ties" in subprocess.run([pkg.database.cli_path(), sub, "--help"], capture_output=True, text=True).stdout

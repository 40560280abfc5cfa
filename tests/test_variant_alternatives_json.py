"""The host-only parts of the variant alternatives: sp_variant_alternatives_json on hand-built records, sp_variant_alt_relations, the layout of the two records and
the switch's bindings.  No device."""
import ctypes as C
import json

import numpy as np
import pytest


def problem(pkg):
    """two haplotypes over variants 0..3 (variant 1 is a sub-allele variant): h0 = {0}, h1 = {0, 1}; calls: 0 hom, 1 and 2 unphased hets, 3 a het with SV label 0"""
    keep = dict(hap_is_sv=np.zeros(2, np.uint8), hap_is_core=np.array([1, 0], np.uint8), slot_off=np.array([0, 1, 3], np.int32),
                alt_off=np.array([0, 1, 2, 3], np.int32), alt_var=np.array([0, 0, 1], np.int32), var_is_core=np.array([1, 0, 1, 1], np.uint8),
                obs_var=np.array([0, 1, 2, 3], np.int32), obs_gt=np.array([4, 1, 1, 1], np.int32), obs_ps=np.full(4, -1, np.int64),
                obs_sv_label=np.array([-1, -1, -1, 0], np.int32))
    p = pkg.ffi.sp_variant_problem()
    p.n_haps, p.n_vars, p.n_obs = 2, 4, 4
    for k, v in keep.items():
        setattr(p, k, v.ctypes.data)
    return p, keep


def record(pkg, score, s0, s1, dip, comb, flags):
    a = pkg.ffi.sp_variant_alt()
    a.score[:] = score
    a.side_score[0][:] = s0
    a.side_score[1][:] = s1
    a.dip[:] = dip
    a.comb, a.flags = comb, flags
    return a


NAMES = dict(hap_names=["*1", "*1.002"], hap_core_names=["*1", "*1"], sv_labels=["*5.001"], var_names=["rs0", "rs1", "rs2", "structural_variant"])


def test_json_fields_in_order(pkg):
    p, _keep = problem(pkg)
    info = pkg.ffi.sp_variant_alt_info()
    info.n_comb, info.n_candidates, info.n_alts, info.n_called = 4, 7, 3, 1
    info.best_score[:] = [0, 0, 0, 0]
    # comb 3: calls 1 and 2 on side 0 (with the hom 0), the SV call 3 on side 1
    alts = [record(pkg, [0, 1, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0], [1, -2], 3, 1),
            record(pkg, [0, 1, 1, 0], [0, 1, 0, 1], [0, 0, 0, 0], [0, -2], 3, 2),
            record(pkg, [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [1, 1], 0, 0)]
    text = pkg.ffi.variant_alternatives_json(p, info, alts, **NAMES)
    doc = json.loads(text, object_pairs_hook=list)
    assert [k for k, _v in doc] == ["n_combinations", "n_candidates", "best_score", "alternatives"]
    doc = json.loads(text)
    assert (doc["n_combinations"], doc["n_candidates"]) == (4, 7)
    assert list(doc["best_score"]) == ["core_missing", "core_unexpected", "sub_missing", "sub_unexpected"] and set(doc["best_score"].values()) == {0}
    first = doc["alternatives"][0]
    assert list(first) == ["rank", "diplotype", "called", "shadowed", "score", "combination", "hap1", "hap2"]
    assert list(first["hap1"]) == ["haplotype", "score", "missing", "unexpected"]
    assert [a["rank"] for a in doc["alternatives"]] == [1, 2, 3]
    assert (first["called"], first["shadowed"], first["combination"]) == (True, False, 3)
    assert first["diplotype"] == "NO_MATCH/NO_MATCH" and first["score"] == {"core_missing": 0, "core_unexpected": 1, "sub_missing": 0, "sub_unexpected": 0}
    assert first["hap1"] == {"haplotype": "*1.002", "score": first["score"], "missing": [], "unexpected": ["rs2"]}
    assert first["hap2"] == {"haplotype": "*5.001", "score": {"core_missing": 0, "core_unexpected": 0, "sub_missing": 0, "sub_unexpected": 0}, "missing": [], "unexpected": []}
    second = doc["alternatives"][1]
    assert (second["called"], second["shadowed"]) == (False, True) and second["hap1"]["unexpected"] == ["rs1", "rs2"]
    # a candidate of score (0, 0, 0, 0) is spelled with the haplotype names, one of (0, 0, ., .) with the core allele names
    assert doc["alternatives"][2]["diplotype"] == "*1.002/*1.002"
    alts[2].score[2] = 1
    assert json.loads(pkg.ffi.variant_alternatives_json(p, info, alts, **NAMES))["alternatives"][2]["diplotype"] == "*1/*1"


def test_json_of_an_empty_list(pkg):
    p, _keep = problem(pkg)
    info = pkg.ffi.sp_variant_alt_info()
    info.n_comb, info.n_candidates, info.n_alts = 4, 0, 0
    info.best_score[:] = [2, 2 ** 63 - 1, 2 ** 63 - 1, 2 ** 63 - 1]
    doc = json.loads(pkg.ffi.variant_alternatives_json(p, info, [], **NAMES))
    assert doc == {"n_combinations": 4, "n_candidates": 0, "alternatives": [],
                   "best_score": {"core_missing": 2, "core_unexpected": None, "sub_missing": None, "sub_unexpected": None}}
    info.n_alts = 1                                # a record that names a haplotype the problem does not have
    with pytest.raises(pkg.StarphaseError):
        pkg.ffi.variant_alternatives_json(p, info, [record(pkg, [0] * 4, [0] * 4, [0] * 4, [2, 0], 0, 0)], **NAMES)


def test_relations_without_a_device(pkg):
    p, _keep = problem(pkg)
    M, U, MI = 1, 2, 3                             # SP_REL_MATCH, SP_REL_UNEXPECTED, SP_REL_MISSING
    rel = pkg.ffi.variant_alt_relations
    # comb 0: every het call on side 1 (bits 0 -> the second haplotype); side 0 holds the hom call only
    assert rel(p, 0, 0, 0) == [(0, M)]
    assert rel(p, 0, 0, 1) == [(0, M), (1, MI)]
    assert rel(p, 0, 1, -2) == [(3, M)]
    # comb 1: call 1 moves to side 0
    assert rel(p, 1, 0, 1) == [(0, M), (1, M)]
    assert rel(p, 1, 0, 0) == [(0, M), (1, U)]
    for bad in ((0, 0, 2), (0, 2, 0), (-1, 0, 0), (4, 0, 0), (0, 0, -1), (0, 0, -2), (0, 1, -3)):      # no such haplotype / side / assignment (n_comb is 4); an SV label the side does not carry
        with pytest.raises(pkg.StarphaseError):
            rel(p, *bad)
    n = C.c_uint32(7)
    ids, out = np.zeros(1, np.int32), np.zeros(1, np.int32)
    assert pkg.ffi.lib().sp_variant_alt_relations(C.byref(p), 4, 0, 0, ids.ctypes.data, out.ctypes.data, 1, C.byref(n)) == pkg.ffi.SP_ERR_INVALID_ARG and n.value == 0
    assert pkg.ffi.lib().sp_variant_alt_relations(C.byref(p), 0, 0, 1, ids.ctypes.data, out.ctypes.data, 1, C.byref(n)) == pkg.ffi.SP_ERR_CAPACITY and n.value == 2


def test_record_layouts(pkg):
    A, I = pkg.ffi.sp_variant_alt, pkg.ffi.sp_variant_alt_info
    assert C.sizeof(A) == 80 and [(f, getattr(A, f).offset) for f, _t in A._fields_] == [("score", 0), ("side_score", 32), ("dip", 64), ("comb", 72), ("flags", 76)]
    assert C.sizeof(I) == 56 and [(f, getattr(I, f).offset) for f, _t in I._fields_] == [("n_comb", 0), ("n_candidates", 8), ("best_score", 16), ("n_alts", 48),
                                                                                        ("n_called", 52)]
    L = pkg.ffi.lib()
    assert L.sp_struct_size(b"sp_variant_alt") == 80 and L.sp_struct_size(b"sp_variant_alt_info") == 56
    assert (pkg.ffi.SP_VAR_ALT_CALLED, pkg.ffi.SP_VAR_ALT_SHADOWED, pkg.ffi.SP_VAR_ALTERNATIVES) == (1, 2, 10)


def test_the_switch_is_bound(pkg):
    assert hasattr(pkg.database._lib(), "sp_starphase_set_variant_alternatives")
    import inspect
    assert "variant_alternatives=False" in inspect.getsource(pkg.database.Starphase.__init__)

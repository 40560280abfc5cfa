"""cyp2d6_alternatives.json as text (sp_cyp_alternatives_json) and the chain list behind index1 / index2 (sp_cyp_possible_chains): host only, no device."""
import ctypes as C
import json

import numpy as np

import cyp_cases
import oracle_ffi as of


def problem(pkg, inp):
    n_reads = max(len(inp.chain_names), len(inp.score_names))
    rco = inp.read_chain_off if len(inp.read_chain_off) == n_reads + 1 else np.zeros(n_reads + 1, np.int32)
    rwo = inp.read_w_off if len(inp.read_w_off) == n_reads + 1 else np.zeros(n_reads + 1, np.int32)
    return pkg.ffi.Context._chain_problem(inp.types, inp.subtypes, inp.cfg["translate"], inp.cfg["connections"], inp.cfg["singletons"], rco, inp.chain_off,
                                          inp.chain_items, rwo, inp.w_ed, inp.w_ov, inp.infer, inp.normalize_all, inp.ignore, inp.penalties)


def alt(pkg, i, j, c1, c2, score, comps, ed, unmet):
    a = pkg.ffi.sp_chain_alt()
    a.index1, a.index2, a.n1, a.n2 = i, j, len(c1), len(c2)
    for x, h in enumerate(c1):
        a.chain1[x] = h
    for x, h in enumerate(c2):
        a.chain2[x] = h
    a.score = score
    a.ln_ed_penalty, a.mn_llh_penalty, a.allele_expected_penalty, a.unexpected_chain_penalty, a.inferred_chain_penalty = comps
    a.edit_distance, a.unmet_observations = ed, unmet
    return a


def render(pkg, p, n_possible, alts, counts, weights, scored=None, cap=None):
    L = pkg.ffi.lib()
    arr = (pkg.ffi.sp_chain_alt * max(1, len(alts)))(*alts)
    need = C.c_uint64(0)
    ns = C.byref(C.c_uint64(scored)) if scored is not None else None
    cp = counts.ctypes.data if counts is not None else None
    wp = weights.ctypes.data if weights is not None else None
    rc = L.sp_cyp_alternatives_json(C.byref(p), n_possible, ns, arr, len(alts), cp, wp, None, 0, C.byref(need))
    assert rc == 0
    size = need.value if cap is None else cap
    buf = C.create_string_buffer(max(1, size))
    rc = L.sp_cyp_alternatives_json(C.byref(p), n_possible, ns, arr, len(alts), cp, wp, buf, size, C.byref(need))
    return rc, need.value, buf.value.decode()


EXPECTED = """{
  "n_possible_chains": 7,
  "alternatives": [
    {
      "rank": 1,
      "diplotype": "*4.001/*10 + *1",
      "chains": [
        [
          "0_CYP2D6*4.001"
        ],
        [
          "1_CYP2D6*1",
          "2_CYP2D6::CYP2D7::exon2",
          "3_CYP2D7"
        ]
      ],
      "score": 12.5,
      "delta_to_best": 0.0,
      "ln_ed_penalty": 4.0,
      "mn_llh_penalty": 8.5,
      "allele_expected_penalty": 0.0,
      "unexpected_chain_penalty": 0.0,
      "inferred_chain_penalty": 0.0,
      "edit_distance": 2,
      "unmet_observations": 0,
      "coverage": [
        {
          "region": "0_CYP2D6*4.001",
          "copies": 1,
          "observed": 10.25
        },
        {
          "region": "1_CYP2D6*1",
          "copies": 1,
          "observed": 9.0
        },
        {
          "region": "2_CYP2D6::CYP2D7::exon2",
          "copies": 1,
          "observed": 0.001
        },
        {
          "region": "3_CYP2D7",
          "copies": 1,
          "observed": 12.0
        }
      ]
    },
    {
      "rank": 2,
      "diplotype": "*4.001x2/*1",
      "chains": [
        [
          "0_CYP2D6*4.001",
          "0_CYP2D6*4.001"
        ],
        [
          "1_CYP2D6*1"
        ]
      ],
      "score": 12.75,
      "delta_to_best": 0.25,
      "ln_ed_penalty": 4.0,
      "mn_llh_penalty": 4.75,
      "allele_expected_penalty": 4.0,
      "unexpected_chain_penalty": 0.0,
      "inferred_chain_penalty": 0.0,
      "edit_distance": 2,
      "unmet_observations": 3,
      "coverage": [
        {
          "region": "0_CYP2D6*4.001",
          "copies": 2,
          "observed": 19.5
        },
        {
          "region": "1_CYP2D6*1",
          "copies": 1,
          "observed": 1e-7
        }
      ]
    }
  ]
}"""


def hand_made(pkg):
    labels = [("CYP2D6", "4.001"), ("CYP2D6", "1"), ("Hybrid", "CYP2D6::CYP2D7::exon2"), ("CYP2D7", None)]
    inp = of.ChainInputs(labels, {}, {}, False, True, of.DEFAULT_PENALTIES, False)
    p, keep = problem(pkg, inp)
    alts = [alt(pkg, 0, 5, [0], [1, 2, 3], 12.5, (4.0, 8.5, 0.0, 0.0, 0.0), 2, 0),
            alt(pkg, 1, 2, [0, 0], [1], 12.75, (4.0, 4.75, 4.0, 0.0, 0.0), 2, 3)]
    counts = np.array([[1, 1, 1, 1], [2, 1, 0, 0]], np.int32)
    weights = np.array([[10.25, 9.0, 0.001, 12.0], [19.5, 1e-7, 3.0, 0.0]], np.float64)
    return p, keep, alts, counts, weights


def test_exact_text_of_two_alternatives(pkg, oracle):
    p, keep, alts, counts, weights = hand_made(pkg)
    rc, need, text = render(pkg, p, 7, alts, counts, weights)
    assert rc == 0 and need == len(text.encode()) + 1
    doc = json.loads(text)
    # the diplotype is convert_chain_to_hap of the two chains at the calls JSON's detail level (the oracle's rendering of the same chains)
    labels = [("CYP2D6", "4.001"), ("CYP2D6", "1"), ("Hybrid", "CYP2D6::CYP2D7::exon2"), ("CYP2D7", None)]
    for e, a in zip(doc["alternatives"], alts):
        want = "/".join(of.chain_hap_string(oracle, list(c[:n]), labels, 1) for c, n in ((a.chain1, a.n1), (a.chain2, a.n2)))
        assert e["diplotype"] == want
    expected = EXPECTED
    for e, k in zip(doc["alternatives"], (1, 2)):                 # (the star strings come from the translation table of the bundled database: taken from the oracle above)
        expected = expected.replace('"diplotype": "%s"' % ("*4.001/*10 + *1" if k == 1 else "*4.001x2/*1"), '"diplotype": "%s"' % e["diplotype"])
    assert text == expected
    rc, need, with_scored = render(pkg, p, 7, alts, counts, weights, scored=21)
    assert rc == 0 and with_scored == expected.replace('"n_possible_chains": 7,\n', '"n_possible_chains": 7,\n  "n_pairs_scored": 21,\n')
    rc, need, bare = render(pkg, p, 7, alts, None, None)
    assert rc == 0 and [e["coverage"] for e in json.loads(bare)["alternatives"]] == [[], []]


def test_needed_protocol_and_empty_list(pkg):
    p, keep, alts, counts, weights = hand_made(pkg)
    rc, need, text = render(pkg, p, 7, alts, counts, weights)
    rc2, need2, cut = render(pkg, p, 7, alts, counts, weights, cap=100)
    assert rc2 == pkg.ffi.SP_ERR_CAPACITY and need2 == need and cut == text[:99]
    rc3, need3, whole = render(pkg, p, 7, alts, counts, weights, cap=need)
    assert rc3 == 0 and whole == text
    rc4, need4, empty = render(pkg, p, 3, [], None, None)
    assert rc4 == 0 and empty == '{\n  "n_possible_chains": 3,\n  "alternatives": []\n}' and need4 == len(empty) + 1
    bad = alt(pkg, 0, 0, [9], [0], 1.0, (0.0, 1.0, 0.0, 0.0, 0.0), 0, 0)          # a region the problem does not have
    arr = (pkg.ffi.sp_chain_alt * 1)(bad)
    assert pkg.ffi.lib().sp_cyp_alternatives_json(C.byref(p), 1, None, arr, 1, None, None, None, 0, C.byref(C.c_uint64(0))) == pkg.ffi.SP_ERR_INVALID_ARG


def test_new_symbols_are_bound(pkg):
    L = pkg.ffi.lib()
    for name in ("sp_cyp_best_chain_pairs", "sp_cyp_possible_chains", "sp_cyp_alternatives_json"):
        assert getattr(L, name).argtypes is not None
    assert hasattr(pkg.database._lib(), "sp_starphase_set_cyp_alternatives")
    assert L.sp_struct_size(b"sp_chain_alt") == C.sizeof(pkg.ffi.sp_chain_alt) == 16 + 2 * 64 * 4 + 6 * 8 + 8 + 8


def test_possible_chains_of_the_reference_scenarios(pkg, oracle):
    """n_chains is the oracle's n_possible and the oracle's winning chains stand at index1 / index2; the cap-and-needed protocol; the expected failure"""
    seen = 0
    for name, inp, status, chains, _ in cyp_cases.reference_cases():
        exp = of.oracle_chain_pair(oracle, inp)
        p, keep = problem(pkg, inp)
        rc, got = pkg.ffi.possible_chains(p)
        assert rc == (16 if status == 16 else 0), name
        if status != 0:
            assert got == []
            continue
        assert len(got) == exp.n_possible, name
        assert sorted([got[exp.index1], got[exp.index2]]) == [list(exp.chain1[:exp.n1]), list(exp.chain2[:exp.n2])], name
        seen += 1
        n_chains, n_items = C.c_uint32(0), C.c_uint32(0)
        off = np.zeros(len(got), np.uint32)                                         # one short of n_chains + 1
        items = np.zeros(sum(len(c) for c in got), np.uint32)
        rc = pkg.ffi.lib().sp_cyp_possible_chains(None, C.byref(p), off.ctypes.data, len(off), items.ctypes.data, len(items), C.byref(n_chains), C.byref(n_items))
        assert rc == pkg.ffi.SP_ERR_CAPACITY and (n_chains.value, n_items.value) == (len(got), len(items))
    assert seen == 6

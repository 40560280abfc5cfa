"""cyp2d6_alternative_reads.json as text (sp_cyp_alternative_reads_json) from hand-made records: host only, no device."""
import ctypes as C
import json

import numpy as np

from chain_pair_reads_cases import chains_of, hand_made, problem
from test_cyp_alternatives_json import alt

NAMES = ["edge", "long", "noobs", "norows", "two"]                     # the reads of hand_made() in problem (name) order


def rec(pkg, rows):
    out = np.zeros((len(rows), len(rows[0])), pkg.ffi.CHAIN_PAIR_READ_DTYPE)
    for k, row in enumerate(rows):
        for r, (excess, supported, m1, m2) in enumerate(row):
            out[k, r]["excess_ed"], out[k, r]["supported"], out[k, r]["mask1"], out[k, r]["mask2"] = excess, supported, m1, m2
            out[k, r]["n_best"] = bin(m1).count("1") + bin(m2).count("1")
    return out


def setup(pkg):
    inp = hand_made()
    p, keep = problem(pkg, inp)
    chains = chains_of(pkg, inp)
    i, j = sorted((chains.index([0, 1]), chains.index([2])))
    h = chains.index([0])
    alts = [alt(pkg, i, j, [0, 1], [2], 3.5, (1.0, 2.5, 0.0, 0.0, 0.0), 8, 1),
            alt(pkg, h, h, [0], [0], 6.0, (2.0, 0.0, 4.0, 0.0, 0.0), 3, 0)]
    #            edge                  long                 noobs         norows        two
    rows = [[(0, 1, 1, 0),         (3, 1, 0b101, 1 << 35), (0, 0, 1, 1), (0, 1, 7, 3), (5, 1, 0, 1)],
            [(2, 1, 1, 1),         (1, 1, 0, 0),           (0, 1, 1, 1), (0, 1, 3, 3), (0, 1, 1, 1)]]
    return inp, p, keep, chains, (i, j), alts, rec(pkg, rows)


def render(pkg, p, alts, recs, names=None, single=(2.0, 0.0, 1.5), cap=None):
    L = pkg.ffi.lib()
    chains, freq, _, edges, weight = pkg.ffi.observed_chains(p)
    off = np.cumsum([0] + [len(c) for c in chains]).astype(np.uint32)
    items = np.array([h for c in chains for h in c] or [0], np.uint32)
    freq = np.ascontiguousarray(freq, np.float64)
    e_from, e_to = np.array([a for a, _ in edges] or [0], np.uint32), np.array([b for _, b in edges] or [0], np.uint32)
    weight = np.ascontiguousarray(weight if len(weight) else [0.0], np.float64)
    single = np.array(single, np.float64)
    arr = (pkg.ffi.sp_chain_alt * max(1, len(alts)))(*alts)
    nm = None
    if names is not None:
        nm = (C.c_char_p * len(names))(*[n.encode() if n is not None else None for n in names])
    need = C.c_uint64(0)

    def call(buf, size):
        return L.sp_cyp_alternative_reads_json(C.byref(p), arr, len(alts), recs.ctypes.data, nm, off.ctypes.data, items.ctypes.data, freq.ctypes.data, len(chains),
                                               single.ctypes.data, e_from.ctypes.data, e_to.ctypes.data, weight.ctypes.data, len(edges), buf, size, C.byref(need))
    assert call(None, 0) == 0
    size = need.value if cap is None else cap
    buf = C.create_string_buffer(max(1, size))
    rc = call(buf, size)
    return rc, need.value, buf.value.decode()


LONG_UNDER_RANK_1 = """        {
          "read": "long",
          "excess_ed": 3,
          "delta_to_best": 0,
          "supported": true,
          "placements": [
            "hap1@0",
            "hap1@2",
            "hap2@35"
          ]
        }"""


def test_the_text_of_two_alternatives(pkg):
    inp, p, keep, chains, (i, j), alts, recs = setup(pkg)
    rc, need, text = render(pkg, p, alts, recs, NAMES)
    assert rc == 0 and need == len(text.encode()) + 1
    doc = json.loads(text)                                                                       # the text parses
    assert list(doc) == ["observed", "alternatives"] and list(doc["observed"]) == ["chains", "regions", "links"]
    obs = doc["observed"]
    assert obs["chains"] == [{"chain": ["0_CYP2D6*1"], "reads": 1.0}, {"chain": ["0_CYP2D6*1", "1_CYP2D6*2"], "reads": 1.0}, {"chain": ["1_CYP2D6*2"], "reads": 1.0},
                             {"chain": ["2_CYP2D6*3"], "reads": 1.0}]
    assert obs["regions"] == [{"region": "0_CYP2D6*1", "reads": 2.0}, {"region": "2_CYP2D6*3", "reads": 1.5}]          # a zero total is left out
    assert obs["links"] == [{"from": "0_CYP2D6*1", "to": "1_CYP2D6*2", "reads": 1.0}]
    assert '"reads": 1.0\n' in text and '"reads": 1.5\n' in text                               # f64 as the other renderers write it
    a, b = doc["alternatives"]
    assert list(a) == ["rank", "diplotype", "chains", "hap1_chain", "edit_distance", "unmet_observations", "reads"]
    assert list(b) == ["rank", "diplotype", "chains", "hap1_chain", "edit_distance", "unmet_observations", "reads_decided_for", "reads_decided_against", "reads"]
    assert (a["rank"], b["rank"]) == (1, 2) and (a["edit_distance"], a["unmet_observations"], b["edit_distance"], b["unmet_observations"]) == (8, 1, 3, 0)
    assert a["chains"] == [["0_CYP2D6*1", "1_CYP2D6*2"], ["2_CYP2D6*3"]] and b["chains"] == [["0_CYP2D6*1"], ["0_CYP2D6*1"]]
    assert a["hap1_chain"] == (1 if chains[i] == [0, 1] else 2) and b["hap1_chain"] == 1
    assert a["diplotype"].count("/") == 1 and b["diplotype"].split("/")[0] == b["diplotype"].split("/")[1]
    # neutral: excess_ed == 0, supported, and the excess of rank 1 -- `edge` and `norows` under rank 1; under rank 2 `noobs` and `norows`, but not `two` (0 against 5)
    assert [r["read"] for r in a["reads"]] == ["long", "noobs", "two"]
    assert [r["read"] for r in b["reads"]] == ["edge", "long", "two"]
    assert LONG_UNDER_RANK_1 in text
    assert a["reads"][1] == {"read": "noobs", "excess_ed": 0, "delta_to_best": 0, "supported": False, "placements": ["hap1@0", "hap2@0"]}
    assert [(r["excess_ed"], r["delta_to_best"]) for r in b["reads"]] == [(2, 2), (1, -2), (0, -5)]               # signed
    assert b["reads"][1]["placements"] == []                                                       # no placement: the read is longer than both chains
    assert (b["reads_decided_for"], b["reads_decided_against"]) == (1, 2)


def test_read_names_and_capacity(pkg):
    inp, p, keep, chains, (i, j), alts, recs = setup(pkg)
    rc, need, text = render(pkg, p, alts, recs, None)
    assert rc == 0 and [r["read"] for r in json.loads(text)["alternatives"][0]["reads"]] == ["read 1", "read 2", "read 4"]
    rc, _, some = render(pkg, p, alts, recs, ["edge", None, "noobs", "norows", "two"])
    assert rc == 0 and [r["read"] for r in json.loads(some)["alternatives"][0]["reads"]] == ["read 1", "noobs", "two"]
    rc2, need2, cut = render(pkg, p, alts, recs, None, cap=100)
    assert rc2 == pkg.ffi.SP_ERR_CAPACITY and need2 == need and cut == text[:99]
    rc3, need3, whole = render(pkg, p, alts, recs, None, cap=need)
    assert rc3 == 0 and whole == text


def test_one_alternative_has_no_decided_fields_and_bad_indices_fail(pkg):
    inp, p, keep, chains, (i, j), alts, recs = setup(pkg)
    rc, need, text = render(pkg, p, alts[:1], recs[:1].copy(), NAMES)
    only, = json.loads(text)["alternatives"]
    assert rc == 0 and "reads_decided_for" not in only and "reads_decided_against" not in only and only["rank"] == 1
    rc, need, none = render(pkg, p, [], recs, NAMES)
    assert rc == 0 and json.loads(none)["alternatives"] == []
    bad = alt(pkg, 0, len(chains), [0], [0], 1.0, (0.0, 1.0, 0.0, 0.0, 0.0), 0, 0)                 # index2 names no chain
    arr = (pkg.ffi.sp_chain_alt * 1)(bad)
    L = pkg.ffi.lib()
    assert L.sp_cyp_alternative_reads_json(C.byref(p), arr, 1, recs.ctypes.data, None, None, None, None, 0, None, None, None, None, 0, None, 0,
                                           C.byref(C.c_uint64(0))) == pkg.ffi.SP_ERR_INVALID_ARG


def test_new_symbols_are_bound(pkg):
    L = pkg.ffi.lib()
    for name in ("sp_cyp_chain_pair_reads", "sp_cyp_observed_chains", "sp_cyp_alternative_reads_json"):
        assert getattr(L, name).argtypes is not None
    assert hasattr(pkg.database._lib(), "sp_starphase_set_cyp_alternative_reads")
    assert L.sp_struct_size(b"sp_chain_pair_read") == C.sizeof(pkg.ffi.sp_chain_pair_read) == pkg.ffi.CHAIN_PAIR_READ_DTYPE.itemsize == 32

"""Problems and helpers shared by the tests of sp_cyp_chain_pair_reads and of sp_cyp_alternative_reads_json; nothing here needs a device."""
import oracle_ffi as of
from test_cyp_alternatives_json import problem  # noqa: F401  (a CPU test module: the sp_chain_problem of a ChainInputs)


def chains_of(pkg, inp):
    p, keep = problem(pkg, inp)
    rc, chains = pkg.ffi.possible_chains(p)                               # host only
    assert rc == 0
    return chains


def hand_made():
    """Regions 0 -> 1 observed, region 2 alone: chains [0], [0, 1], [1], [2].  `long`: two rows -- longer than both chains of ([0], [2]), longer than one of
    ([0, 1], [2]); `noobs`: no observed chain; `norows`: an observed chain and no weight rows."""
    H = 3
    row = lambda *ed: [(e, 0.25 + 0.125 * x) for x, e in enumerate(ed)]
    obs = {"edge": [[0, 1]], "long": [[0]], "noobs": [], "norows": [[1]], "two": [[2]]}
    sc = {"edge": [row(0, 3, 3), row(3, 0, 3)], "long": [row(1, 4, 2), row(5, 1, 7)], "noobs": [row(2, 0, 1)], "norows": [], "two": [row(3, 3, 0)]}
    return of.ChainInputs([("CYP2D6", str(h + 1)) for h in range(H)], obs, sc, False, True, of.DEFAULT_PENALTIES, True)

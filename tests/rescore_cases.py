"""Designed pairs for the re-score shortcuts of sp_rescore_mappings (af_classify_kernel, sp_affine.hip): every query is its target with planted edits, placed where
the classification changes its mind -- AF_ISOLATED = 16 bases between edits and from the ends, AF_MARGIN = 24 around a cluster, AF_MAXMID + 1 = 16 stretches,
the 64 bases of K1's ends_only, the crossing of the two gap pieces at 20 bases.  A plain builder: no GPU, no fixtures.  The reference of every test that uses it
is oracle/affine.c (tests/oracle_ffi.py oracle_affine).

A batch is a list of Case, pair i = (targets[i], queries[i]).  route / route_ends name the route a case was built for (0 closed form, 1 the DP over the rows
around the clusters, 2 the DP over all rows, 3 no mapping; None: not pinned, e.g. an edit the unit-cost cell may spell either way) with ends_only = 0 and
windows = 1, and with ends_only = 64; a dict {band: route} where the band decides."""
import numpy as np

AF_ISOLATED, AF_MARGIN, AF_MAXMID = 16, 24, 15
BASES = "ACGT"
MAX_ED = 200                     # covers the longest planted gap (100) and the fullest fuzz read
EVENTS_STRIDE = 256


class Case:
    def __init__(self, family, target, query, diag=0, route=None, route_ends=None, bands=(64, 256), max_ed=MAX_ED, clean=None, place=None, route_ends_a5=None):
        self.family, self.target, self.query = family, target, query
        self.diag = diag                 # t_pos - q_pos handed to the cell: midway between the diagonals of the two ends
        self.route, self.route_ends, self.bands, self.max_ed = route, route_ends, bands, max_ed
        self.spelled_as_planted = False                # the CPU design test checks that the unit-cost cell spells the pair's edits as they were planted
        self.clean, self.place = clean, place          # clusters behind a clean end: the clean bases, and which end(s)
        self.route_ends_a5 = route_ends if route_ends_a5 is None else route_ends_a5       # ends_only with match score 5, where the score an end must keep is another


def _no_repeat(rng, n, before=None, after=None):
    """n random bases, no two neighbours equal (an indel then has one place only), none equal to the base before / after the stretch"""
    out, prev = [], before
    for k in range(n):
        ban = {prev} | ({after} if k == n - 1 else set())
        c = BASES[int(rng.integers(0, 4))]
        while c in ban:
            c = BASES[int(rng.integers(0, 4))]
        out.append(c); prev = c
    return "".join(out)


def _other(rng, *ban):
    c = BASES[int(rng.integers(0, 4))]
    while c in ban:
        c = BASES[int(rng.integers(0, 4))]
    return c


def apply_edits(rng, target, edits):
    """edits = [(pos, kind, n)] on the target: 'X' another base at pos, 'I' n bases the target does not have in front of pos, 'D' n bases from pos on missing, 'N' an N at pos.
    -> (query, bases inserted - bases deleted)"""
    q, shift = list(target), 0
    for pos, kind, n in sorted(edits, key=lambda e: -e[0]):
        if kind == "X":                          # (not a neighbour's base either: a cluster of mismatches then has no cheaper spelling with gaps)
            q[pos] = _other(rng, target[pos], target[pos - 1] if pos > 0 else None, target[pos + 1] if pos + 1 < len(target) else None)
        elif kind == "N":
            q[pos] = "N"
        elif kind == "I":
            q[pos:pos] = list(_no_repeat(rng, n, target[pos - 1] if pos > 0 else None, target[pos] if pos < len(target) else None)); shift += n
        else:
            del q[pos:pos + n]; shift -= n
    return "".join(q), shift


CLUSTERS = {"6 on every second base": [0, 2, 4, 6, 8, 10], "6 consecutive": [0, 1, 2, 3, 4, 5], "8 on every third base": [0, 3, 6, 9, 12, 15, 18, 21]}


def _case(rng, family, L, edits, **kw):
    t = _no_repeat(rng, L)
    q, shift = apply_edits(rng, t, edits)
    c = Case(family, t, q, diag=-(shift // 2) if shift >= 0 else (-shift) // 2, **kw)
    c.edits = sorted(edits)
    return c


def designed(seed=20260):
    rng = np.random.default_rng(seed)
    cases = []
    length = lambda: int(rng.integers(400, 1201))
    # ---- lone edits
    for kind in "XID":
        for d in (1, 8, 15, 16, 17, 24, 40):
            for place in ("head", "tail", "both"):
                L = length()
                e = ([(d, kind, 1)] if place in ("head", "both") else []) + ([(L - 1 - d if kind != "I" else L - d, kind, 1)] if place in ("tail", "both") else [])
                r = 0 if d >= AF_ISOLATED else None
                cases.append(_case(rng, "lone", L, e, route=r, route_ends=r))
    # ---- two edits mid-sequence
    for k1 in "XID":
        for k2 in "XID":
            for s in (1, 2, 15, 16, 17):
                L = length(); p = L // 2
                if s <= 2: r = 1 if k1 == k2 else None
                elif s == 15: r = None if k1 == "I" else 1
                elif s == 16: r = None if k1 == "D" else 0
                else: r = 0
                cases.append(_case(rng, "two edits", L, [(p, k1, 1), (p + s, k2, 1)], route=r))
    # ---- clusters behind a clean end (two targets each), and the same clusters mid-sequence
    for name, offs in CLUSTERS.items():
        for clean in (15, 16, 17, 20, 24, 30, 40, 63, 64, 65):
            for place in ("head", "tail", "both"):
                for _rep in range(2):
                    L = length(); e = []
                    if place in ("head", "both"): e += [(clean + o, "X", 1) for o in offs]
                    if place in ("tail", "both"): e += [(L - 1 - clean - o, "X", 1) for o in offs]
                    # every such cluster takes the rows around it; ends_only: an end with a clustered edit within 64 bases takes the DP over its stretch (a mismatch
                    # `clean` bases before the tail lies clean + 1 bases from the alignment's end), the others are cleared by their score (64 - 24 >= 8)
                    near = clean <= 63 if place in ("head", "both") else clean <= 62
                    # (six consecutive mismatches have spellings with gaps at the same or a lower unit cost, whose outermost edit lies a few bases off: not pinned at 63 - 65)
                    planted = name != "6 consecutive"
                    cases.append(_case(rng, "cluster behind a clean end", L, e, clean=clean, place=place, route=1, route_ends=(1 if near else 0) if planted or clean <= 40 else None))
                    cases[-1].spelled_as_planted = planted
        L = length()
        cases.append(_case(rng, "cluster mid-sequence", L, [(L // 2 + o, "X", 1) for o in offs], route=1, route_ends=0))
    # ---- long gaps (the two gap pieces cross at 20 bases), mid-sequence and 30 bases from an end
    for kind in "ID":
        for n in (2, 7, 13, 19, 20, 21, 40, 100):
            bands = (64, 256) if n <= 21 else (256,)
            L = length()
            cases.append(_case(rng, "long gap", L, [(L // 2, kind, n)], route=1, bands=bands))
            L = length()
            cases.append(_case(rng, "long gap", L, [(30, kind, n)], bands=bands))
            L = length()
            cases.append(_case(rng, "long gap", L, [(L - 30 - (n if kind == "D" else 0), kind, n)], bands=bands))
    # ---- stretch geometry
    pair = lambda p: [(p, "X", 1), (p + 1, "X", 1)]
    for sep in (39, 40, 41, 2 * AF_MARGIN + 15, 2 * AF_MARGIN + 16, 2 * AF_MARGIN + 17):          # clean bases between two clusters: one stretch or two
        L = length(); p = L // 3
        cases.append(_case(rng, "two clusters", L, pair(p) + pair(p + 2 + sep), route=1, route_ends=0))
    L = 1200; e = []                                              # 18 clusters, each a stretch of its own: more than AF_MAXMID + 1
    for k in range(18):
        e += pair(38 + k * (2 + 2 * AF_MARGIN + AF_ISOLATED))
    cases.append(_case(rng, "18 clusters", L, e, route=1, route_ends=1))            # (ends_only: the first and the last one lie within 64 bases of an end: two stretches)
    for d in (17, 20, 23, 25):                                    # the first stretch would begin before the alignment does
        L = length()
        cases.append(_case(rng, "cluster at the head", L, pair(d) + pair(L // 2), route=1, route_ends=1))
    for n in (70, 90):                                            # a gap that takes both ends out of the 64 diagonals around the middle one: no stretch fits that band
        L = length()
        cases.append(_case(rng, "does not fit", L, pair(100) + [(L // 2, "D", n)] + pair(L - 100), route={64: 2, 256: 1}, route_ends={64: 2, 256: None}))
    for place in ("head", "tail", "both"):                        # 20 mismatches on every second base, 65 clean bases from an end: beyond the 64 bases, so the score decides.  (The cell spells so heavy a cluster
    # with gaps, in fewer edits than planted: which way the score falls is not pinned, the extents are held to the oracle.)
        L = length(); e = []
        if place in ("head", "both"): e += [(65 + 2 * o, "X", 1) for o in range(20)]
        if place in ("tail", "both"): e += [(L - 1 - 65 - 2 * o, "X", 1) for o in range(20)]
        cases.append(_case(rng, "score boundary", L, e, route=1))
    L = 420; e = []                                               # ends_only: the stretches of the two ends meet
    for p in range(20, L - 20, 30):
        e += pair(p)
    cases.append(_case(rng, "head and tail meet", L, e, route_ends=2))
    for where in ("start", "end", "both"):                       # queries that overhang the target
        L = length(); t = _no_repeat(rng, L)
        q, _ = apply_edits(rng, t, pair(L // 2) + [(60, "X", 1)])
        h = _no_repeat(rng, 60, None, t[0]) if where in ("start", "both") else ""
        tl = _no_repeat(rng, 60, t[-1], None) if where in ("end", "both") else ""
        cases.append(Case("overhang", t, h + q + tl, diag=-len(h), route=1, route_ends=0))
        cases.append(Case("overhang", h + q + tl, t, diag=len(h), route=1, route_ends=0))                     # ... and targets that overhang the query
    c = _case(rng, "no mapping", 400, pair(200), route=3, route_ends=3); c.max_ed = -1
    cases.append(c)
    return cases


def with_n(seed=20261):
    """an N in the query, in the target, in both: a set that holds one has no closed form and no stretches -- a batch of its own"""
    rng = np.random.default_rng(seed)
    cases = []
    for where in ("query", "target", "both"):
        for extra in ([], [(150, "X", 1)], [(150, "X", 1), (152, "D", 1)]):
            L = int(rng.integers(400, 1201)); t = _no_repeat(rng, L)
            q, shift = apply_edits(rng, t, extra + ([(L // 2, "N", 1)] if where in ("query", "both") else []))
            if where in ("target", "both"):
                t = t[:L // 3] + "N" + t[L // 3 + 1:]
            cases.append(Case("N in both" if where == "both" else "N in the " + where, t, q, diag=0, route=2, route_ends=2))
    return cases


FUZZ_PAIRS = 1500


def fuzz(n=FUZZ_PAIRS, seed=20262):
    """reads of 300 - 900 bases: 0 - 4 clusters of 2 - 10 edits over 4 - 30 bases, 0 - 6 lone edits, one end in three with a cluster within 70 bases"""
    rng = np.random.default_rng(seed)
    cases = []
    for _ in range(n):
        L = int(rng.integers(300, 901))
        t = "".join(BASES[c] for c in rng.integers(0, 4, L))
        spots = {}
        def cluster(lo):
            span, ne = int(rng.integers(4, 31)), int(rng.integers(2, 11))
            for p in rng.integers(lo, lo + span, ne):
                spots[int(p)] = "XID"[int(rng.integers(0, 3))]
        for _c in range(int(rng.integers(0, 5))):
            cluster(int(rng.integers(1, L - 32)))
        if rng.integers(0, 3) == 0: cluster(int(rng.integers(1, 41)))
        if rng.integers(0, 3) == 0: cluster(L - 32 - int(rng.integers(1, 41)))
        for _l in range(int(rng.integers(0, 7))):
            spots[int(rng.integers(1, L - 1))] = "XID"[int(rng.integers(0, 3))]
        q, shift = apply_edits(rng, t, [(p, k, 1) for p, k in spots.items()])
        cases.append(Case("fuzz", t, q, diag=-(shift // 2) if shift >= 0 else (-shift) // 2, max_ed=MAX_ED))
    return cases


def expected_route(case, band, windows, ends_only, a=1):
    """the route a case names for these knobs, or None"""
    r = (case.route_ends_a5 if a == 5 else case.route_ends) if ends_only else case.route
    if isinstance(r, dict): r = r[band]
    if r == 1 and not windows: r = 2
    return r

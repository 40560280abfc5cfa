"""Brute force for sp_variant_alternatives: every candidate (het assignment, explanation of side 0, explanation of side 1) of a variant problem, scored with the
oracle's osp_quant_match through variant_glue.het_split / quant_match, ordered by the definition in include/starphase_hip.h.  Plain Python over the problem's
arrays; nothing of the library is used."""
import variant_glue as vg

MAX = 2 ** 63 - 1
CALLED, SHADOWED = 1, 2


def n_combinations(prob):
    """(n_comb, n_sides) as solve_diplotype counts them: one bit per phase set (first seen) and per unphased het, the last bit fixed"""
    n_obs = len(prob.obs)
    groups, seen, hets = 0, set(), 0
    for o in range(n_obs):
        if prob.obs_gt[o] == 4:
            continue
        hets += 1
        ps = int(prob.obs_ps[o])
        if ps >= 0:
            if ps not in seen:
                seen.add(ps)
                groups += 1
        else:
            groups += 1
    return (1 << (groups - 1), 2) if hets else (1, 1)


class Brute:
    def __init__(self, oracle, prob):
        self.oracle, self.prob = oracle, prob
        n_obs = len(prob.obs)
        self.label_of = {int(prob.obs_var[o]): int(prob.obs_sv[o]) for o in range(n_obs)}
        self.n_comb, self.n_sides = n_combinations(prob)
        self._cells = {}
        self.sv_sides = self.ineligible_sides = 0
        cands, solve = [], []                      # solve: per assignment (total as the solve sees it, kept explanations per side or None)
        self.n_candidates = 0
        for comb in range(self.n_comb):
            lists = vg.het_split(prob, comb)[:self.n_sides]
            sides = [self.explain(ids) for ids in lists]
            best, kept = [], []
            for ex in sides:
                if not ex:
                    best.append((1, MAX, MAX, MAX))
                    kept.append([])
                    continue
                b = min(s for s, _d in ex)
                at = [d for s, d in ex if s == b]
                if any(d >= 0 and not prob.hap_is_core[d] for d in at):          # sub-alleles shadow core alleles
                    at = [d for d in at if d < 0 or not prob.hap_is_core[d]]
                best.append(b)
                kept.append(at)
            total = best[0] if self.n_sides == 1 else tuple(MAX if MAX in (a, b) else a + b for a, b in zip(best[0], best[1]))
            solve.append((total, kept))
            if not all(sides):
                self.ineligible_sides += 1
                continue
            if self.n_sides == 1:
                self.n_candidates += len(sides[0])
                cands += [(s, comb, d, d, s, s) for s, d in sides[0]]
            else:
                self.n_candidates += len(sides[0]) * len(sides[1])
                cands += [(tuple(a + b for a, b in zip(s0, s1)), comb, d0, d1, s0, s1) for s0, d0 in sides[0] for s1, d1 in sides[1]]
        cands.sort(key=lambda c: c[:4])
        self.best_score = min(t for t, _k in solve)
        called = set()
        for comb, (t, kept) in enumerate(solve):
            if t != self.best_score or MAX in t:
                continue
            if self.n_sides == 1:
                called |= {(comb, d, d) for d in kept[0]}
            else:
                called |= {(comb, d0, d1) for d0 in kept[0] for d1 in kept[1]}
        self.n_called = len(called)
        self.records = []
        for total, comb, d0, d1, s0, s1 in cands:
            flags = 0
            if total == self.best_score:
                flags = CALLED if (comb, d0, d1) in called else SHADOWED
            self.records.append((total, s0, s1, d0, d1, comb, flags))

    def cell(self, h, ids):
        key = (h, tuple(ids))
        if key not in self._cells:
            core = self.prob.var_is_core
            _m, mi, e = vg.quant_match(self.oracle, self.prob, h, ids)
            self._cells[key] = (sum(1 for v in mi if core[v]), sum(1 for v in e if core[v]), sum(1 for v in mi if not core[v]), sum(1 for v in e if not core[v]))
        return self._cells[key]

    def explain(self, ids):
        """[(side score, dip)] of one side's variant list"""
        labels = [self.label_of[v] for v in ids if self.label_of[v] >= 0]
        if labels:
            self.sv_sides += 1
            return [((0, len(set(labels[1:])), 0, 0), -(labels[0] + 2))]
        out = []
        for h in range(len(self.prob.haps)):
            if self.prob.hap_is_sv[h]:
                continue
            s = self.cell(h, ids)
            if s[0] <= 1:
                out.append((s, h))
        return out

    def top(self, n):
        return self.records[:n]


def gpu_records(alts):
    """sp_variant_alt structs -> the tuples of Brute.records"""
    return [(tuple(a.score), tuple(a.side_score[0]), tuple(a.side_score[1]), a.dip[0], a.dip[1], a.comb, a.flags) for a in alts]

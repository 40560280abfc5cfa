"""The CPU reference of sp_hla_map_ties: the class of every allowed allele of a consensus against a scan's winner, from ALIGNMENTS and CIGARs alone (never from
the device's event rows or level records).

Each level's record is built the way the reference builds an HlaProcessedMatch (src/hla/processed_match.rs:53-100): the prefix-edit array is osp_process_mm_cigar
of oracle/liboracle.so on the mapping's CIGAR, the range and the stats are add_mapping's (k2_levels_kernel states the same rule).  The two directions are
osp_is_better_match(W, X) and osp_is_better_match(X, W) of the same library -- both functions are bound here, with ctypes.  Whether a direction was decided in the
level loop (:113-168) or only by the final mapping_score comparison (:174-183) is found by checking the overlap edit counts and the presence rule again, in Python.

  0 distinct   1 score_only   2 equal   3 beats_winner   4 winner          (include/starphase_hip.h, sp_hla_map_ties)"""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISTINCT, SCORE_ONLY, EQUAL, BEATS_WINNER, WINNER = range(5)
EVENT_ROW = 255                    # the event-row cap of both scans: a mapping with more edit bases is no mapping to the a = 5 scan (include/starphase_hip.h, best_mm2)


class Level(C.Structure):          # osp_hla_level (oracle/sp_oracle.h)
    _fields_ = [("present", C.c_int32), ("range_start", C.c_int32), ("range_end", C.c_int32),
                ("len", C.c_int32), ("nm", C.c_int32), ("unmapped", C.c_int32), ("pc", C.POINTER(C.c_uint64))]


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
        L.osp_process_mm_cigar.restype = C.c_int32
        L.osp_process_mm_cigar.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
        L.osp_is_better_match.restype = C.c_int32
        L.osp_is_better_match.argtypes = [C.POINTER(Level * 2), C.POINTER(Level * 2)]
        _lib = L
    return _lib


def score_value(length, nm, unmapped):
    """src/data_types/mapping.rs:191-195"""
    return max(float(nm + unmapped), 0.1) / float(length)


class Record:
    """one level of one allele: absent, or a mapping (ops = [(len, op)] with 7 '=', 8 'X', 1 'I' allele only, 2 'D' consensus only; a = allele, b = consensus)"""

    def __init__(self, ops=None, a_start=0, a_end=0, b_start=0, b_end=0, a_len=0, b_len=0):
        self.present = False
        self.pc = None
        if ops is None:
            return
        nm = sum(n for n, op in ops if op in (1, 2, 8))
        unmapped = a_len - (a_end - a_start)
        if not score_value(a_len, nm, unmapped) < 1.0:               # select_best_mapping has to beat its (1, 1, 0) default (caller.rs:1447-1461)
            return
        clip_start, clip_end = a_start, a_len - a_end
        ln = np.array([n for n, _op in ops], np.uint32)
        op = np.array([o for _n, o in ops], np.uint8)
        self.pc = np.zeros(b_len + 1, np.uint64)
        rc = lib().osp_process_mm_cigar(ln.ctypes.data, op.ctypes.data, len(ops), b_start, b_len, clip_start, clip_end, self.pc.ctypes.data)
        assert rc == 0, rc
        self.present = True
        self.range_start = max(b_start - clip_start, 0)
        self.range_end = b_end + min(clip_end, b_len - b_end)
        self.len, self.nm, self.unmapped = a_len, nm, unmapped

    def level(self):
        lv = Level()
        if self.present:
            lv.present, lv.range_start, lv.range_end, lv.len, lv.nm, lv.unmapped = 1, self.range_start, self.range_end, self.len, self.nm, self.unmapped
            lv.pc = self.pc.ctypes.data_as(C.POINTER(C.c_uint64))
        return lv


def better(x, w):
    """osp_is_better_match(x, w) for two (cDNA record, DNA record) pairs"""
    lx, lw = (Level * 2)(x[0].level(), x[1].level()), (Level * 2)(w[0].level(), w[1].level())
    return bool(lib().osp_is_better_match(C.byref(lx), C.byref(lw)))


def decided_in_level_loop(x, w):
    """does the level loop of is_better_match return for this pair (in either direction: its conditions are symmetric), or does it fall through to the mapping score"""
    for a, b in zip(x, w):
        if a.present and b.present:
            os_, oe = max(a.range_start, b.range_start), min(a.range_end, b.range_end)
            if os_ < oe and int(a.pc[oe]) - int(a.pc[os_]) != int(b.pc[oe]) - int(b.pc[os_]):
                return True
        elif a.present or b.present:
            return True
    return False


def classify(records, winner):
    """records[k] = (cDNA Record, DNA Record) of allowed allele k; winner = the scan's winner as an index into records, or -1 -> (uint8 classes, counts[5])"""
    n = len(records)
    cls = np.zeros(n, np.uint8)
    if winner < 0:
        return cls, np.zeros(5, np.uint32)
    w = records[winner]
    for k in range(n):
        if k == winner:
            cls[k] = WINNER
            continue
        b_wx, b_xw = better(w, records[k]), better(records[k], w)
        if b_xw:
            cls[k] = BEATS_WINNER
        elif not b_wx:
            cls[k] = EQUAL
        else:
            cls[k] = DISTINCT if decided_in_level_loop(records[k], w) else SCORE_ONLY
    return cls, np.bincount(cls, minlength=5).astype(np.uint32)


def scan_winner(records):
    """score_read's strict running best over the records in order (caller.rs:1411-1500) -> index or -1"""
    absent = (Record(), Record())
    best, at = absent, -1
    for k, r in enumerate(records):
        if better(r, best):
            best, at = r, k
    return at


def records_from_map(m, allele_len):
    """the a = 5 scan's records of an HlaMap (HlaDb.map_consensus*): the map's handed-out alignments and CIGARs.  allele_len(level, allele) = the allele's length at
    that level.  A mapping with more than EVENT_ROW edit bases is absent, as the scan has it."""
    out = []
    for k, a in enumerate(m.alleles):
        pair = []
        for lv in (0, 1):
            al = m.aln[lv, k]
            b_len = len(m.cons_cdna if lv == 0 else m.cons_dna)
            if int(al["score"]) <= 0 or int(al["nm"]) > EVENT_ROW:
                pair.append(Record())
                continue
            ops = [(int(w) >> 4, int(w) & 15) for w in m.cigar[lv][k]]
            pair.append(Record(ops, int(al["a_start"]), int(al["a_end"]), int(al["b_start"]), int(al["b_end"]), allele_len(lv, int(a)), b_len))
        out.append(tuple(pair))
    return out


def ops_from_events(aln, ev):
    """an alignment of the cell contract (sp_aln + its event words, type << 30 | b_pos in path order; X 0, D 1 consumes the consensus, I 2 the allele) -> [(len, op)]"""
    steps, j = [], int(aln["b_start"])
    for e in ev[:int(aln["nm"])]:
        t, pos = int(e) >> 30, int(e) & 0x3FFFFFFF
        if pos > j:
            steps.append((pos - j, 7)); j = pos
        steps.append((1, (8, 2, 1)[t]))
        if t != 2:
            j += 1
    if int(aln["b_end"]) > j:
        steps.append((int(aln["b_end"]) - j, 7))
    ops = []
    for n, op in steps:
        if ops and ops[-1][1] == op:
            ops[-1] = (ops[-1][0] + n, op)
        else:
            ops.append((n, op))
    return ops


def records_from_cells(ctx, alleles, seqs_of_level, cons_of_level, min_votes=2, max_ed=EVENT_ROW):
    """the unit-cost scan's records: the map does not hand out the library's unit-cost alignments per allele, so the same pairs go through the public cell contract --
    Context.anchor_batch for the diagonal (K2 runs a pair whose anchor has at least 2 votes) and Context.align_batch (sp_align_batch, events on) for the alignment --
    and the records are built from THOSE alignments.  alleles: database indices; seqs_of_level[lv][a] / cons_of_level[lv]: strings ('' = none at that level)"""
    per_level = []
    for lv in (0, 1):
        recs = [Record() for _ in alleles]
        cons = cons_of_level[lv]
        have = [k for k, a in enumerate(alleles) if seqs_of_level[lv][int(a)]]
        if cons and have:
            A = ctx.upload([seqs_of_level[lv][int(alleles[k])] for k in have])
            B = ctx.upload([cons])
            idx = np.arange(len(have), dtype=np.uint32)
            diag, votes = ctx.anchor_batch(B, A, np.zeros(len(have), np.uint32), idx)        # allele_pos - cons_pos
            run = [x for x in range(len(have)) if votes[x] >= min_votes]
            if run:
                aln, ev = ctx.align_batch(A, B, np.array(run, np.uint32), np.zeros(len(run), np.uint32), -diag[run], max_ed, events=True)
                for y, x in enumerate(run):
                    if aln[y]["ok"]:
                        al = aln[y]
                        recs[have[x]] = Record(ops_from_events(al, ev[y]), int(al["a_start"]), int(al["a_end"]), int(al["b_start"]), int(al["b_end"]), int(al["a_len"]), int(al["b_len"]))
        per_level.append(recs)
    return list(zip(per_level[0], per_level[1]))

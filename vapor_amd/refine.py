"""Breakpoint refinement (`vapor bed | vcf --refine M[:T]`; not in the reference): a call whose
breakpoints are tens of bases off - every short-read call set, every VCF record with CIPOS / CIEND - is scored at a grid of
candidate breakpoints around the called ones, on one window with one set of reads, and the row reports the best candidate.

This module holds the candidate model, the pick rule and the brute-force route (one ordinary Score request per candidate,
the host finish, the pick in Python): the statement the batched route (pipeline.score_grids, grid_pick_kernel) is tested
against, and the route of a library without the device step (the CPU twin of the C ABI).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L

MAX_CANDIDATES = L.MAX_CANDIDATES        # one wavefront holds a locus with two candidates per lane


def default_step(margin: int) -> int:
    """The step when none is given: the smallest T whose grid reaches the margin within MAX_CANDIDATES candidates,
    (2 * ceil(M / T) + 1) ** 2 <= MAX_CANDIDATES - 10 for a margin of 50 (121 candidates).  (With M // T in place of the
    ceiling the smallest step for 50 would be 9, whose grid ends at +-45 and holds no multiple of 10; an explicit step is
    held to the cap alone, (2 * (M // T) + 1) ** 2 <= MAX_CANDIDATES.)"""
    t = 1
    while (2 * -(-margin // t) + 1) ** 2 > MAX_CANDIDATES:
        t += 1
    return t


def parse(spec: str) -> Tuple[int, int]:
    """'M' or 'M:T' -> (M, T); ValueError for anything else, and for a step whose grid exceeds MAX_CANDIDATES."""
    parts = str(spec).split(":")
    try:
        if len(parts) not in (1, 2):
            raise ValueError
        m = int(parts[0])
        t = int(parts[1]) if len(parts) == 2 else None
    except ValueError:
        raise ValueError("--refine takes M or M:T (margin and step in bp), not %r" % (spec,)) from None
    if m < 0 or (t is not None and t < 1):
        raise ValueError("--refine %s: the margin is an integer >= 0, the step an integer >= 1" % spec)
    if t is None:
        return m, default_step(m)
    n = (2 * (m // t) + 1) ** 2
    if n > MAX_CANDIDATES:
        raise ValueError("--refine %s: %d candidates per locus, at most %d (the smallest step for this margin is %d)"
                         % (spec, n, MAX_CANDIDATES, default_step(m)))
    return m, t


def _moves(margin: int, step: int, ci=None) -> List[int]:
    lo, hi = -margin, margin
    if ci is not None:
        lo, hi = max(lo, int(ci[0])), min(hi, int(ci[1]))
    j = margin // step
    return [d * step for d in range(-j, j + 1) if lo <= d * step <= hi or d == 0]


def candidates(margin: int, step: int, s: int, e: int, cipos=None, ciend=None) -> List[Tuple[int, int]]:
    """The candidate moves (ds, de) of a call [s, e]: multiples of `step` in [-margin, margin] (within CIPOS / CIEND where the
    record has them; 0 always), a = s + ds, b = e + de with b - a >= 1, ordered by (|ds| + |de|, |ds|, ds, de): candidate 0 is
    the call itself, a lower index a smaller move."""
    out = [(ds, de) for ds in _moves(margin, step, cipos) for de in _moves(margin, step, ciend) if (e + de) - (s + ds) >= 1 or (ds, de) == (0, 0)]
    out.sort(key=lambda c: (abs(c[0]) + abs(c[1]), abs(c[0]), c[0], c[1]))
    return out


# ------------------------------------------------------------------------------------------
# a candidate's record and the choice among them
# ------------------------------------------------------------------------------------------

def record(scores: Sequence[Optional[float]]) -> np.ndarray:
    """The eight doubles finish_kernel writes for a locus (VAPOR_LOCUS_STRIDE: QS, GS, GT index, GQ, reads scored, positive
    scores, scores that round to <= 0, 0; all NaN but [4] = 0 without a scored read) from its per-read scores (None or NaN: a
    skipped read), with the host's float64 steps (vapor_amd.finish)."""
    from . import finish
    s = np.asarray([x for x in scores if x is not None and x == x], dtype=np.float64)
    out = np.full(L.LOCUS_STRIDE, np.nan)
    n = int(s.size)
    if n == 0:
        out[4] = 0.0
        return out
    pos = s[s > 0]
    npos = int(pos.size)
    nnon = int(finish.rounded_nonpositive(s).sum())
    qs = float(np.mean(pos)) if npos else 0.0
    gs = float(npos) / float(n)
    gt, gq = 1, np.nan
    if n < L.GT_TABLE_N:
        gt, gq = int(finish.gt_table()[n, nnon, 0]), finish.gt_table()[n, nnon, 1]
    if gt == 0 and gs > .15:
        gt = 1
    out[:] = (qs, gs, float(gt), gq, float(n), float(npos), float(nnon), 0.0)
    return out


def _key(v: float):
    """A NaN never beats a number (`nan > x` is false in vapor_amd.finish's tests too); -0.0 is 0.0."""
    return (0, 0.0) if v != v else (1, float(v) + 0.0)


def pick(table) -> int:
    """The winner among the candidates' records ((n, 8) doubles, candidate 0 first): a candidate is eligible when it scored at
    least one read and at least as many as candidate 0 ([4] > 0 and [4] >= table[0][4]); among the eligible the largest GS
    wins, then the largest QS, then the lowest index; candidate 0 when none is eligible."""
    t = np.asarray(table, dtype=np.float64).reshape(-1, L.LOCUS_STRIDE)
    n0 = t[0, 4]
    best, best_key = 0, None
    for c in range(len(t)):
        if not (t[c, 4] > 0 and t[c, 4] >= n0):
            continue
        key = (_key(t[c, 1]), _key(t[c, 0]))
        if best_key is None or key > best_key:
            best, best_key = c, key
    return best


class GridResult:
    """The answer to a drivers.ScoreGrid: `winner` (index among the candidates), `rec` / `rec0` (the winner's and candidate
    0's eight doubles), `scores` (the winner's per-read scores, None for a skipped read); with want_all also every
    candidate's record (`all_recs`, (n, 8)) and per-read scores (`all_scores`)."""
    __slots__ = ("winner", "rec", "rec0", "scores", "all_recs", "all_scores")

    def __init__(self, winner, rec, rec0, scores, all_recs=None, all_scores=None):
        self.winner, self.rec, self.rec0, self.scores = int(winner), rec, rec0, scores
        self.all_recs, self.all_scores = all_recs, all_scores


def score_grid_brute(engine, req):
    """The brute-force route for one ScoreGrid request: an ordinary Score request per candidate through
    pipeline.score_requests, the host finish per candidate (record), the pick in Python.  Returns a GridResult, or the
    exception a candidate's request ended with."""
    from . import pipeline
    from .drivers import Score
    outs = pipeline.score_requests(engine, [Score(req.kind, req.ref_seq, alt, req.reads, req.k) for alt in req.alts])
    for v in outs:
        if isinstance(v, BaseException):
            return v
    recs = np.stack([record(v) for v in outs])
    w = pick(recs)
    return GridResult(w, recs[w], recs[0], list(outs[w]), recs, [list(v) for v in outs])


class Refined(list):
    """A refined locus's score list (the winner's), with what the extra columns need: `info` = five floats - the winner's
    breakpoints a and b, candidate 0's QS and GS on the widened window (NaN where it scored no read) and its number of
    positive scores."""
    info = None


INFO = (
    ("VaPoR_RPOS", "Integer", "1", "Start of the best-scoring candidate breakpoint pair (--refine)"),
    ("VaPoR_REND", "Integer", "1", "End of the best-scoring candidate breakpoint pair (--refine)"),
    ("VaPoR_QS0", "Float", "1", "VaPoR_QS of the called breakpoints on the widened window (--refine)"),
    ("VaPoR_GS0", "Float", "1", "VaPoR_GS of the called breakpoints on the widened window (--refine)"),
)
COLUMNS = tuple(i[0] for i in INFO)


def pack(info) -> List[float]:
    """`info` as it travels between ranks (a second table of "scores"): its five floats, none for a locus that was not refined."""
    return list(info or ())


def unpack(flat):
    return flat if flat is not None and len(flat) else None


def columns(info) -> List[str]:
    """The four extra fields of a row: the winner's a and b, candidate 0's QS and GS the way the row's own QS and GS are
    written (finish.row_tail: 0 without a positive score, NA without a scored read); four '.' for a locus that was not
    refined (info None or empty)."""
    if info is None or len(info) == 0:
        return ["."] * 4
    a, b, qs0, gs0, npos0 = [float(v) for v in info]
    if gs0 != gs0:
        return [str(int(a)), str(int(b)), "NA", "NA"]
    return [str(int(a)), str(int(b)), "0" if npos0 == 0 else str(qs0), str(gs0)]


def columns_many(infos) -> List[List[str]]:
    return [columns(info) for info in infos]

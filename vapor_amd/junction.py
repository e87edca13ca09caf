"""`vapor bed | vcf --realign --realign-polish --realign-junction`: the event the polished allele carries.  The
polished alt allele is read as one jump away from the reference window - a forward pass from the common window start and a
backward pass from the common window end meet at the jump, which may be of any length - and the jump is held against the jump
of the call's own allele.  This module is the rule, checked exactly: `row_table`, `junction` and `lens` (the Python statement
the two kernels of vapor_junction.h are held to, with realign.statement's rows) - and the mode's surface for cli.py and the VCF
writer (INFO, COLUMNS, pack, unpack, columns_many: polish's, followed by six columns).  The device finds the jumps
(Engine.realign_junction; pipeline.realign_requests makes the call); there is no other route.  No record is edited."""
from __future__ import annotations

from typing import List

import numpy as np

from . import polish, realign

NONE, DEL, INS = range(3)                                            # the type of a lens
TYPES = ("NONE", "DEL", "INS")
COST0, LEFT0, RIGHT0, GLEN0, COST, LEFT, RIGHT, GLEN, TYPE = range(9)  # what a locus's Junction holds

_INFO = (
    ("VaPoR_RA_JT", "String", "1", "The event the polished alt allele carries against its window: DEL, INS or NONE (--realign-junction)"),
    ("VaPoR_RA_JLEN", "Integer", "1", "Length of that event (--realign-junction)"),
    ("VaPoR_RA_JLEN0", "Integer", "1", "Length of the event of the call's own alt allele, by the same rule (--realign-junction)"),
    ("VaPoR_RA_JDL", "Integer", "1", "Left end of the polished allele's event minus that of the call's, in bases (--realign-junction)"),
    ("VaPoR_RA_JDR", "Integer", "1", "Right end of the polished allele's event minus that of the call's, in bases (--realign-junction)"),
    ("VaPoR_RA_JCOST", "Integer", "1", "Edits the polished allele still has against its best one-jump reading (--realign-junction)"),
)

_BIG = 1 << 28                 # a cell that does not exist


def _rows(a: np.ndarray, b: np.ndarray, band: int):
    """(f, jf) of the bases `a` (ns) against `b` (nl >= ns): realign.statement's rows with off2 = 0, and behind every row the
    minimum of D over the row's existing cells, at the smallest j."""
    band = int(band)
    if not 1 <= band <= realign.MAX_BAND:
        raise ValueError("junction: band %d outside 1 .. %d" % (band, realign.MAX_BAND))
    n, m, w = len(a), len(b), 2 * band + 1
    if n > m:
        raise ValueError("junction: the first sequence (%d symbols) is longer than the second (%d)" % (n, m))
    c = np.arange(w, dtype=np.int64)
    bpad = np.full(n + m + 2 * w + 2, realign._NEVER_B, dtype=np.int64)   # b[j - 1] of slot c in row i stands at bpad[i - 1 + c]
    bpad[band:band + m] = b
    j = c - band
    row = np.where((j >= 0) & (j <= m), j, _BIG)
    f = np.zeros(n + 1, dtype=np.int64)
    jf = np.zeros(n + 1, dtype=np.int64)
    big1 = np.full(1, _BIG, dtype=np.int64)
    for i in range(1, n + 1):
        cell = (c >= band - i) & (c <= m + band - i)                     # 0 <= j = i + c - band <= m
        diag = row + (bpad[i - 1:i - 1 + w] != a[i - 1])
        vert = np.concatenate((row[1:], big1)) + 1
        t = np.where(cell, np.minimum(diag, vert), _BIG)
        row = np.where(cell, np.minimum(np.minimum.accumulate(t - c) + c, _BIG), _BIG)
        k = int(np.argmin(row))                                          # (the first minimum: the smallest slot, the smallest j)
        f[i], jf[i] = row[k], k + i - band
    return f, jf


def row_table(s, l, band: int):
    """T(s, l): (f, jf), two int64 arrays of len(s) + 1 rows.  f[i] is the minimum of D[i][j] over the existing cells of row i
    (|i - j| <= band, 0 <= j <= len(l)), D of s[0:i] against l[0:j] anchored at (0, 0) with realign's symbols and unit costs;
    jf[i] the smallest j that attains it.  len(s) <= len(l)."""
    return _rows(realign._bases(s, realign._NEVER_A), realign._bases(l, realign._NEVER_B), band)


def junction(s, l, band: int, want_rows: bool = False):
    """(cost, i, j1, j2, f_F(i), f_R(ns - i)) of the pair (s, l), len(s) <= len(l): with F = T(s, l) and R = T(reversed s,
    reversed l), split row i has j1 = jf_F(i), j2 = nl - jf_R(ns - i), cost = f_F(i) + f_R(ns - i) and is valid iff j2 >= j1;
    the valid row with the smallest (cost, i).  s is l with l[j1:j2] skipped at row i.  With want_rows also the (ns + 1, 4)
    rows {f_F, jf_F, f_R, jf_R}, each pass's pair indexed by its own row."""
    a, b = realign._bases(s, realign._NEVER_A), realign._bases(l, realign._NEVER_B)
    ff, jff = _rows(a, b, band)
    fr, jfr = _rows(a[::-1], b[::-1], band)
    ns, nl = len(a), len(b)
    j1, j2, cost = jff, nl - jfr[::-1], ff + fr[::-1]
    i = int(np.argmin(np.where(j2 >= j1, cost, _BIG)))                   # (the first minimum: the leftmost row)
    got = (int(cost[i]), i, int(j1[i]), int(j2[i]), int(ff[i]), int(fr[ns - i]))
    return (got, np.stack((ff, jff, fr, jfr), axis=1).astype(np.int32)) if want_rows else got


def of_record(rec, deletion_form: bool):
    """(cost, left, right, glen, type) of a pair's record {status, cost, i, j1, j2, ..} as Engine.realign_junction and `junction`
    (behind a 0) give it: the deletion form where the allele was the pair's shorter sequence, else the insertion form."""
    cost, i, j1, j2 = (int(v) for v in rec[1:5])
    glen = j2 - j1
    if deletion_form:
        return cost, j1, j2, glen, DEL if glen > 0 else NONE
    return cost, i, i, glen, INS if glen > 0 else NONE


def deletion_form(allele_len: int, window_len: int) -> bool:
    """Whether an allele is read as its window with a stretch skipped (it is not the longer of the two)."""
    return int(allele_len) <= int(window_len)


def lens(allele, window, band: int):
    """(cost, left, right, glen, type) of an allele on its window, left and right in window coordinates.  Deletion form
    (len(allele) <= len(window)): the junction of (allele, window), left = j1, right = j2, DEL when glen > 0.  Insertion form:
    the junction of (window, allele), left = right = i, INS when glen > 0.  NONE when glen == 0."""
    if deletion_form(len(allele), len(window)):
        return of_record((0,) + junction(allele, window, band), True)
    return of_record((0,) + junction(window, allele, band), False)


class Junction:
    """What `--realign-junction` knows of a locus: the lens of the call's own allele and of the polished allele, nine integers
    {cost0, left0, right0, glen0, cost, left, right, glen, type}.  Rides on the locus's realign.Payload as `.junction`, beside
    `.polish`; travels in the gather."""
    __slots__ = ("vals",)

    def __init__(self, vals):
        self.vals = tuple(int(v) for v in vals)
        if len(self.vals) != 9:
            raise ValueError("junction: a locus holds nine integers")


def applies(p) -> bool:
    """Whether the lens applies to a payload: it has a pile of status 0 with at least MIN_COV reads, both pairs came back (it
    carries a Junction) and the call's own allele is exactly one jump of its window (cost0 == 0)."""
    if p is None or p.polish is None or p.junction is None:
        return False
    return p.polish.stats[polish.STATUS] == 0 and p.polish.stats[polish.PAIRS] >= polish.MIN_COV and p.junction.vals[COST0] == 0


def six(p) -> List[str]:
    """The six columns behind polish's: '.' where the lens does not apply."""
    if not applies(p):
        return ["."] * 6
    v = p.junction.vals
    return [TYPES[v[TYPE]], str(v[GLEN]), str(v[GLEN0]), str(v[LEFT] - v[LEFT0]), str(v[RIGHT] - v[RIGHT0]), str(v[COST])]


# (the section: the nine integers travel; and the surface of a run with `--realign-junction`, polish's columns then the six)
SECTION = realign.Section("junction", _INFO, six, lambda jn: jn.vals, lambda flat, at: (Junction(flat[at:at + 9]), at + 9))
SECTIONS = polish.SECTIONS + (SECTION,)
_CHAIN = realign.Chain(SECTIONS)
INFO, COLUMNS = _CHAIN.INFO, _CHAIN.COLUMNS
columns, pack, unpack, columns_many = _CHAIN.columns, _CHAIN.pack, _CHAIN.unpack, _CHAIN.columns_many

"""`vapor bed | vcf --realign --realign-polish`: the traces of a locus's ALT voters stacked on the alt allele,
column by column, and the allele the reads carry.  This module is the rule - constants and integer comparisons, checked exactly:
`statement` (the Python statement the four kernels of vapor_polish.h are held to, built on realign.trace_statement), `apply`
(the polished allele as text) - and the mode's surface for cli.py and the VCF writer (INFO, COLUMNS, pack, unpack,
columns_many: realign's, followed by six columns).  The device piles (Engine.realign_polish; pipeline.realign_requests makes the
call); there is no other route."""
from __future__ import annotations

from typing import List, Optional

import numpy as np

from . import realign

MIN_COV = 3                    # a column, or a boundary between two columns, is judged from this many pairs on
RMAX = 64                      # inserted bases kept per site
MAX_SITES = 256                # insertion sites kept per locus, in column order

KEEP, DELETE, SITE_BIT = 4, 5, 8                                     # the call byte: 0 .. 3 a substituted base, KEEP, DELETE; | SITE_BIT
A, C, G, T, O, DL, BCOV, INS = range(8)                              # a column's counters
STATUS, PAIRS, PCOV, PSUB, PDEL, SITES, PINS, DROPPED = range(8)     # a locus's statistics

_INFO = (
    ("VaPoR_RA_PN", "Integer", "1", "Reads that vote for the alt allele and are piled on it (--realign-polish)"),
    ("VaPoR_RA_PCOV", "Integer", "1", "Columns of the alt allele that at least 3 piled reads cover (--realign-polish)"),
    ("VaPoR_RA_PSUB", "Integer", "1", "Columns where a strict majority of the piled reads holds another base (--realign-polish)"),
    ("VaPoR_RA_PDEL", "Integer", "1", "Columns that a strict majority of the piled reads deletes (--realign-polish)"),
    ("VaPoR_RA_PINS", "Integer", "1", "Bases that a strict majority of the piled reads inserts (--realign-polish)"),
    ("VaPoR_RA_PID", "Float", "1", "Identity of the alt allele to the piled reads, 1 - (PSUB + PDEL + PINS) / PCOV (--realign-polish)"),
)


def statement(reads_with_off2, allele, band: int):
    """(counts, calls, sites, ins, stats) of a locus: `allele` of len symbols, columns 0 .. len - 1, and its pairs [(read, off2)].
    counts (len, 8) uint32, a column's A C G T O Dl bcov ins; calls (len) uint8; sites (MAX_SITES, 2) int32, a kept site's
    (column, bases); ins (MAX_SITES, RMAX) uint8, its text in upper case and 0 behind it; stats 8 int32 {0, pairs, PCOV, PSUB,
    PDEL, sites kept, PINS, sites dropped}.
    A pair's trace (realign.trace_statement) is walked from (0, 0), i read symbols and j allele symbols consumed, the column of
    allele symbol j being off2 + j.  A leading 'D' run of `lead` is no coverage (realign.fold_leading_d): the pair covers
    off2 + lead .. off2 + j_end - 1.  '=' / 'X': + 1 on the read symbol's base, O for a symbol that is none.  A later 'D': + 1
    on Dl.  Every covered column but the pair's first: + 1 on bcov.  An 'I' run of L before column q counts iff
    off2 + lead < q < off2 + j_end: + 1 on ins of q."""
    len_a = len(allele)
    counts = np.zeros((len_a, 8), dtype=np.uint32)
    walks = []                                                        # per pair its counted 'I' runs: (column, read bases of the run)
    for read, off2 in reads_with_off2:
        off2 = int(off2)
        _d, _i_end, j_end, runs = realign.trace_statement(read, allele, off2, band)
        rb = realign._bases(read, O)
        lead, rest = realign.fold_leading_d(runs)
        first_col, end_col = off2 + lead, off2 + j_end
        i, j, mine = 0, lead, []
        for k, op in rest:
            if op == "I":
                q = off2 + j
                if first_col < q < end_col:
                    counts[q, INS] += 1
                    mine.append((q, rb[i:i + k]))
                i += k
                continue
            for s in range(k):
                col = off2 + j + s
                counts[col, DL if op == "D" else int(rb[i + s])] += 1
                if col != first_col:
                    counts[col, BCOV] += 1
            j += k
            if op != "D":
                i += k
        walks.append(mine)
    ab = realign._bases(allele, KEEP)
    calls = np.full(len_a, KEEP, dtype=np.uint8)
    stats = np.zeros(8, dtype=np.int32)
    stats[PAIRS] = len(walks)
    sites = np.zeros((MAX_SITES, 2), dtype=np.int32)
    ins = np.zeros((MAX_SITES, RMAX), dtype=np.uint8)
    slot_of = {}
    for q in range(len_a):
        row = [int(v) for v in counts[q]]
        cov = sum(row[:6])
        if cov >= MIN_COV:
            stats[PCOV] += 1
            cand = row[:4] + [row[DL]]
            best = max(cand)
            if 2 * best > cov:                                        # a strict majority is unique
                w = cand.index(best)
                if w == 4:
                    calls[q] = DELETE
                    stats[PDEL] += 1
                elif w != int(ab[q]):
                    calls[q] = w
                    stats[PSUB] += 1
        if q >= 1 and row[BCOV] >= MIN_COV and 2 * row[INS] > row[BCOV]:
            if len(slot_of) < MAX_SITES:
                slot_of[q] = len(slot_of)
                sites[slot_of[q], 0] = q
                calls[q] |= SITE_BIT
            else:
                stats[DROPPED] += 1
    stats[SITES] = len(slot_of)
    insb = np.zeros((max(len(slot_of), 1), RMAX, 4), dtype=np.int64)
    for mine in walks:
        for q, bases in mine:
            if q in slot_of:
                for r, b in enumerate(bases[:RMAX]):
                    if b < 4:
                        insb[slot_of[q], r, int(b)] += 1
    for q, s in slot_of.items():
        bcov = int(counts[q, BCOV])
        for r in range(RMAX):
            if not 2 * int(insb[s, r].sum()) > bcov:
                break
            ins[s, r] = ord("ACGT"[int(np.argmax(insb[s, r]))])       # (argmax: the smallest code on a tie)
            sites[s, 1] += 1
        stats[PINS] += int(sites[s, 1])
    return counts, calls, sites, ins, stats


def apply(allele_text: str, calls, sites, ins) -> str:
    """The polished allele: column by column the inserted bases of the site before it, in upper case, then the column's own
    byte for KEEP (case kept), the called base in upper case for a substitution, nothing for DELETE."""
    out, slot = [], 0
    for q, ch in enumerate(str(allele_text)):
        call = int(calls[q])
        if call & SITE_BIT:
            out.append(bytes(bytearray(int(v) for v in ins[slot][:int(sites[slot][1])])).decode("latin-1"))
            slot += 1
        call &= 7
        if call == KEEP:
            out.append(ch)
        elif call < 4:
            out.append("ACGT"[call])
    return "".join(out)


class Polish:
    """What `--realign-polish` knows of a locus: its eight statistics, and on the rank that scored it, where a sink takes it, the
    polished allele as text.  Rides on the locus's realign.Payload as `.polish`; the statistics travel in the gather, the text
    does not."""
    __slots__ = ("stats", "text")

    def __init__(self, stats, text=None):
        self.stats, self.text = tuple(int(v) for v in stats), text


def identity(stats) -> Optional[str]:
    """VaPoR_RA_PID of a locus's statistics; None when no column is covered."""
    pcov = int(stats[PCOV])
    return "%.4f" % (1 - (int(stats[PSUB]) + int(stats[PDEL]) + int(stats[PINS])) / pcov) if pcov else None


def six(p) -> List[str]:
    """The six columns behind realign's: '.' without a payload, without a pile, or for a locus whose status is not 0."""
    if p is None or p.polish is None or p.polish.stats[STATUS] != 0:
        return ["."] * 6
    s = p.polish.stats
    return [str(s[PAIRS]), str(s[PCOV]), str(s[PSUB]), str(s[PDEL]), str(s[PINS]), identity(s) or "."]


# (the section: the eight statistics travel; and the surface of a run with `--realign-polish` alone, realign's columns then the six)
SECTION = realign.Section("polish", _INFO, six, lambda po: po.stats, lambda flat, at: (Polish(flat[at:at + 8]), at + 8))
SECTIONS = (SECTION,)
_CHAIN = realign.Chain(SECTIONS)
INFO, COLUMNS = _CHAIN.INFO, _CHAIN.COLUMNS
columns, pack, unpack, columns_many = _CHAIN.columns, _CHAIN.pack, _CHAIN.unpack, _CHAIN.columns_many


class PolishWriter(realign.TraceWriter):
    """The sink of `--realign --realign-polish --realign-out PREFIX`: realign.TraceWriter - PREFIX.fa and PREFIX.sam byte for
    byte - and PREFIX.pol.fa beside them: per locus with a payload `>KEY|POL` and the polished allele on one line, in job
    order, with PREFIX.fa's #2, #3 rule for a repeated key."""

    def __init__(self, prefix: str, rank: int = 0, world: int = 1):
        super().__init__(prefix, rank, world)
        self._polished = {}

    def take(self, order: int, key: str, payload) -> None:
        super().take(order, key, payload)
        po = payload.polish if payload is not None else None
        if po is not None and po.text is not None:
            with self._lock:
                self._polished[int(order)] = (key, po.text)

    def close(self):
        names = super().close()
        with open(self.stem + ".pol.fa", "w") as f:
            f.write("".join(">%s|POL\n%s\n" % kt for kt in realign.numbered(self._polished)))
        self._polished = {}
        return names + (self.stem + ".pol.fa",)

"""`vapor bed | vcf --realign`: every read of a locus aligned to the reference allele and to the alt allele, and
the allele it fits better.  This module is the rule - the edit distance of a read against an allele inside a band, start anchored
at the window start, both ends free (`statement`, the Python statement the kernel is held to), a read's vote (`votes`), a locus's
payload and columns (`payload`, `columns`) - and the mode's surface for cli.py and the VCF writer (INFO, COLUMNS, pack, unpack,
columns_many).  The device computes the distances (realign_kernel through Engine.realign; pipeline.realign_requests makes the
call); there is no other route.  The genotype of the two counts is support.genotype's, so that VaPoR_RA_GT and VaPoR_SUP_GT are
comparable."""
from __future__ import annotations

from typing import List, Optional

import numpy as np

from . import support

BAND = 256                     # the band of the command line: a cell (i, j) exists iff |i - j| <= BAND
MAX_BAND = 512                 # the widest band the kernel takes (VAPOR_MAX_BAND)
MARGIN = 10                    # a read votes when its two distances differ by at least this (the smallest event the drivers take is
                               # 50 bp, whose expected difference is about the event's length): a rule, not a tolerance

INFO = (
    ("VaPoR_RA_ALT", "Integer", "1", "Reads that align better to the alt allele, by at least 10 edits (--realign)"),
    ("VaPoR_RA_REF", "Integer", "1", "Reads that align better to the reference allele, by at least 10 edits (--realign)"),
    ("VaPoR_RA_NC", "Integer", "1", "Reads whose two alignments differ by fewer than 10 edits: no call (--realign)"),
    ("VaPoR_RA_VAF", "Float", "1", "Allele fraction of the reads, VaPoR_RA_ALT / (VaPoR_RA_ALT + VaPoR_RA_REF) (--realign)"),
    ("VaPoR_RA_GT", "String", "1", "Genotype of the reads: the likeliest of 0/0, 0/1 and 1/1 at an error rate of 0.05 (--realign)"),
    ("VaPoR_RA_GQ", "Integer", "1", "Quality of VaPoR_RA_GT: ten times the log10 likelihood ratio to the second genotype, at most 99 (--realign)"),
    ("VaPoR_RA_Rec", "Integer", ".", "Per read, its edit distance to the reference allele minus that to the alt allele (--realign)"),
)
COLUMNS = tuple(i[0] for i in INFO)

_NEVER_A, _NEVER_B = 4, 5      # the base of a symbol that matches nothing, in the read and in the allele: never equal
_BIG = 1 << 28                 # a cell that does not exist


def _bases(seq, never: int) -> np.ndarray:
    """Per symbol its base 0 .. 3 (A C G T in either case), `never` for everything else (N, IUPAC, any other byte)."""
    table = np.full(256, never, dtype=np.int64)
    for v, ch in enumerate("ACGT"):
        table[ord(ch)] = table[ord(ch.lower())] = v
    raw = seq.encode("latin-1") if isinstance(seq, str) else bytes(seq)
    return table[np.frombuffer(raw, dtype=np.uint8)]


def statement(read, allele, off2: int, band: int) -> int:
    """d of the pair (read, allele, off2) inside `band`: a = read (n symbols), b = allele[off2:] (m symbols); D[0][0] = 0; a cell
    (i, j) exists iff 0 <= i <= n, 0 <= j <= m and |i - j| <= band; D[i][j] = the minimum over its existing predecessors of
    D[i-1][j-1] + (0 if a[i-1] matches b[j-1] else 1), D[i-1][j] + 1, D[i][j-1] + 1; d = the minimum of D over the existing cells
    of the last row and of the last column.  Two symbols match iff both are A, C, G or T in either case and the same base.
    One row of the band at a time: slot c = j - i + band, so the diagonal predecessor is the same slot of the row before and the
    vertical one slot c + 1; the horizontal steps of a row are a running minimum of t[c] - c."""
    band, off2 = int(band), int(off2)
    if not 1 <= band <= MAX_BAND:
        raise ValueError("realign: band %d outside 1 .. %d" % (band, MAX_BAND))
    if not 0 <= off2 <= len(allele):
        raise ValueError("realign: off2 %d outside 0 .. %d" % (off2, len(allele)))
    a = _bases(read, _NEVER_A)
    b = _bases(allele, _NEVER_B)[off2:]
    n, m, w = len(a), len(b), 2 * band + 1
    c = np.arange(w, dtype=np.int64)
    bpad = np.full(n + m + 2 * w + 2, _NEVER_B, dtype=np.int64)      # b[j - 1] of slot c in row i stands at bpad[i - 1 + c]
    bpad[band:band + m] = b
    j = c - band
    row = np.where((j >= 0) & (j <= m), j, _BIG)
    col = m + band                                                    # the slot of column m in row i is col - i
    d = int(row[col]) if 0 <= col < w else _BIG
    for i in range(1, n + 1):
        j = c + (i - band)
        diag = row + (bpad[i - 1:i - 1 + w] != a[i - 1])
        vert = np.append(row[1:], _BIG) + 1
        t = np.where((j >= 0) & (j <= m), np.minimum(diag, vert), _BIG)
        row = np.minimum(np.minimum.accumulate(t - c) + c, _BIG)
        s = col - i
        if 0 <= s < w:
            d = min(d, int(row[s]))
    d = min(d, int(row.min()))
    return d


def votes(d_ref, d_alt) -> List[int]:
    """Per read its diff = d_ref - d_alt: the read votes ALT iff diff >= MARGIN, REF iff diff <= -MARGIN, else it makes no call."""
    return [int(r) - int(a) for r, a in zip(d_ref, d_alt)]


def counts(diffs):
    """(ALT, REF, NC) of a list of diffs."""
    alt = sum(1 for v in diffs if v >= MARGIN)
    ref = sum(1 for v in diffs if v <= -MARGIN)
    return alt, ref, len(diffs) - alt - ref


class Payload(list):
    """The reads' diffs, in read order."""

    def __init__(self, diffs=()):
        super().__init__(int(v) for v in diffs)


def payload(d_ref, d_alt, status_ref=None, status_alt=None) -> Optional[Payload]:
    """A locus's payload from its reads' two distances; None when a pair came back with a status."""
    for st in (status_ref, status_alt):
        if st is not None and any(int(v) != 0 for v in st):
            return None
    return Payload(votes(d_ref, d_alt))


def columns(p) -> List[str]:
    """The seven columns of a payload as text; every one '.' for a locus without a payload."""
    if p is None:
        return ["."] * 7
    alt, ref, nc = counts(p)
    gt, gq = support.genotype(alt, ref)
    return [str(alt), str(ref), str(nc), "%.3f" % (alt / (alt + ref)) if alt + ref else ".", gt if gt is not None else ".",
            str(gq) if gt is not None else ".", ",".join(str(v) for v in p) if len(p) else "."]


def pack(p) -> List[float]:
    """The payload as floats for the gather across ranks: the number of reads, then their diffs (all far below 2^53: exact);
    nothing for a locus without one."""
    if p is None:
        return []
    return [float(len(p))] + [float(v) for v in p]


def unpack(flat) -> Optional[Payload]:
    if flat is None or len(flat) == 0:
        return None
    return Payload(flat[1:1 + int(flat[0])])


def columns_many(payloads) -> List[List[str]]:
    return [columns(p) for p in payloads]

"""`vapor bed | vcf --depth`: read depth inside a DEL or TANDUP call against the depth of its flanks, a second
line of evidence beside the dot plots of the reads that cross a breakpoint.  This module is the rule - the intervals of a locus
(`regions`), what a record covers (`cover`), the fold change and its verdict (`fold`) - and the mode's surface for cli.py and
the VCF writer (INFO, COLUMNS, pack, unpack, columns_many).  The readers that apply the rule to a BAM file are
seqio.*.depth_many: bam_depth_kernel on the device, vapor_bam_depth on the host, `cover` over bamio's records; what they need to
know of this module is its reader surface (ROW_WIDTH .. locus_payload below)."""
from __future__ import annotations

from typing import List, Optional

W = 1000                       # bases of each flank
P = 10000                      # bases probed at each end of an event longer than 2 * P
EXCLUDE = 0x704                # never counted: unmapped, secondary, QC-fail, duplicate (`samtools depth`)
DEL_BELOW, DUP_ABOVE = (7, 10), (13, 10)     # the fold change supports a DEL below 0.7, a TANDUP above 1.3 (duphold's DHFFC)
TYPES = ("DEL", "TANDUP")

INFO = (
    ("VaPoR_DP_IN", "Float", "1", "Mean read depth inside the event, at its two ends for an event above 20 kb (--depth)"),
    ("VaPoR_DP_FL", "Float", "1", "Mean read depth of the 1 kb flanks of the event (--depth)"),
    ("VaPoR_DFC", "Float", "1", "Fold change of read depth, inside over flanks (--depth)"),
    ("VaPoR_DSUP", "Integer", "1", "1 if the fold change supports the call, below 0.7 for DEL and above 1.3 for TANDUP, else 0 (--depth)"),
)
COLUMNS = tuple(i[0] for i in INFO)

# The reader surface: a region's row as the readers take it - its integers, the indices of its walk window -, the answer of a
# region without records and the answer's type; the library's host and device entry, the Engine's method, the BamFile's and the
# backends'.  LINKED: whether a region has a partner contig and its records carry FLAG and the SA value.  ASKED_WITHOUT_CHUNKS:
# whether the native reader asks the library about a region no chunk overlaps - here it does not: such a region is zeros.
ROW_WIDTH, WINDOW, ZERO, DTYPE = 4, (0, 3), (0, 0, 0), "uint64"
ENTRIES, DEVICE, NATIVE, MANY = ("vapor_bam_depth", "vapor_bam_depth_device"), "bam_depth_device", "depth_native", "depth_many"
LINKED = ASKED_WITHOUT_CHUNKS = False

_COVERS = (1, 0, 0, 0, 0, 0, 0, 1, 1)        # M I D N S H P = X: covers the reference bases it spans
_ADVANCES = (1, 0, 1, 1, 0, 0, 0, 1, 1)      # ... moves the reference cursor


def regions(svtype: str, info, contig_len: int) -> list:
    """The depth regions of a record `info` = [chrom, s, e] (1-based inclusive) of type `svtype` on a contig of contig_len
    bases: a list of (b0, b1, b2, b3), 0-based, cutting left flank [b0, b1), inside [b1, b2) and right flank [b2, b3) - one
    region for an event of at most 2 * P bases, two (each end's P bases with its flank) for a longer one, none for a type
    that is not measured.  Every bound is clipped to [0, contig_len]."""
    if svtype not in TYPES:
        return []
    s, e = int(info[1]), int(info[2])
    length = e - s + 1
    if length <= 2 * P:
        raw = [(s - 1 - W, s - 1, e, e + W)]
    else:
        raw = [(s - 1 - W, s - 1, s - 1 + P, s - 1 + P), (e - P, e - P, e, e + W)]
    n = max(int(contig_len), 0)
    out = []
    for r in raw:
        b = [min(max(x, 0), n) for x in r]
        for k in (1, 2, 3):                   # (clipping keeps the order; an event with e < s is left with empty intervals)
            b[k] = max(b[k], b[k - 1])
        out.append(tuple(b))
    return out


def cover(records, bounds) -> list:
    """[cov0, cov1, cov2] of the records over the three intervals of `bounds` = (b0, b1, b2, b3): the sum, over every record's
    M, = and X operations, of the operation's overlap with the interval.  records: (pos, ops) pairs, pos the 1-based POS and
    ops the operations as uint32 (length << 4 | code) - what bamio.BamFile.fetch_raw gives; the caller has applied the filter."""
    b0, b1, b2, b3 = [int(x) for x in bounds]
    iv = ((b0, b1), (b1, b2), (b2, b3))
    cov = [0, 0, 0]
    for pos, ops in records:
        cur = int(pos) - 1
        for o in (ops.tolist() if hasattr(ops, "tolist") else ops):
            code, n = o & 15, o >> 4
            if code > 8:
                continue
            if _COVERS[code]:
                for i, (lo, hi) in enumerate(iv):
                    a, z = max(cur, lo), min(cur + n, hi)
                    if z > a:
                        cov[i] += z - a
            if _ADVANCES[code]:
                cur += n
    return cov


def statement(records, row, partner=None, min_mapq=0) -> list:
    """The Python statement the readers are held to: a region's words from its records (pos, ops)."""
    return cover(records, row)


def merge_words(a, b) -> list:
    """The answers of one region from two files of a per-chromosome pattern: summed."""
    return [int(x) + int(y) for x, y in zip(a, b)]


def locus_regions(svtype: str, locus, length_of) -> list:
    """A locus's regions as the chunk hook sends them: [(contig, bounds, None)]; length_of(contig): the contig's length."""
    return [(locus[0], b, None) for b in regions(svtype, locus, length_of(locus[0]))] if svtype in TYPES else []


def locus_payload(svtype: str, locus, regs, answers) -> Optional["Payload"]:
    """The locus's Payload from locus_regions' list and the regions' words; None for a locus that is not measured."""
    p = payload(svtype, [b for _c, b, _p in regs], answers)
    return Payload(p, svtype) if p is not None else None


def parse_cigar(text: str) -> list:
    """A CIGAR text as `cover`'s operations ('*' and '' : none)."""
    import re
    return [(int(n) << 4) | "MIDNSHP=X".index(c) for n, c in re.findall(r"(\d+)([MIDNSHP=X])", text or "")]


def payload(svtype: str, regs, covs) -> Optional[list]:
    """A locus's payload [cov_in, len_in, cov_fl, len_fl] from its regions and their three sums each; None for a locus that is
    not measured."""
    if svtype not in TYPES or not regs:
        return None
    cov_in = len_in = cov_fl = len_fl = 0
    for (b0, b1, b2, b3), c in zip(regs, covs):
        cov_in += int(c[1])
        len_in += b2 - b1
        cov_fl += int(c[0]) + int(c[2])
        len_fl += (b1 - b0) + (b3 - b2)
    return [cov_in, len_in, cov_fl, len_fl]


def fold(svtype: str, p) -> list:
    """The four columns of a payload: DP_IN, DP_FL, DFC, DSUP as text.  The fold change is compared as an exact ratio of
    integers, not as its printed text."""
    if p is None:
        return ["."] * 4
    cov_in, len_in, cov_fl, len_fl = [int(x) for x in p]
    if len_in == 0:
        return ["."] * 4
    dp_in = "%.2f" % (cov_in / len_in)
    dp_fl = "%.2f" % (cov_fl / len_fl) if len_fl else "."
    if len_fl == 0 or cov_fl == 0:
        return [dp_in, dp_fl, ".", "."]
    num, den = cov_in * len_fl, cov_fl * len_in
    if svtype == "DEL":
        sup = num * DEL_BELOW[1] < den * DEL_BELOW[0]
    else:
        sup = num * DUP_ABOVE[1] > den * DUP_ABOVE[0]
    return [dp_in, dp_fl, "%.3f" % (num / den), "1" if sup else "0"]


class Payload(list):
    """[cov_in, len_in, cov_fl, len_fl] with the locus's type, which decides the verdict."""
    svtype = "DEL"

    def __init__(self, values, svtype="DEL"):
        super().__init__(int(v) for v in values)
        self.svtype = svtype


def pack(p) -> List[float]:
    """The payload as floats for the gather across ranks: the four integers (below 2^53: exact) and the type, 0 for DEL and 1
    for TANDUP; nothing for a locus without one."""
    if p is None:
        return []
    return [float(v) for v in p] + [float(TYPES.index(getattr(p, "svtype", "DEL")))]


def unpack(flat) -> Optional[Payload]:
    if flat is None or len(flat) == 0:
        return None
    return Payload(flat[:4], TYPES[int(flat[4])] if len(flat) > 4 else "DEL")


def columns_many(payloads) -> List[List[str]]:
    return [fold(getattr(p, "svtype", "DEL"), p) for p in payloads]

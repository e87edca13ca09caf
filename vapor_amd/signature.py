"""`vapor bed | vcf --signatures`: split-read and CIGAR evidence per call - how many alignments are clipped at a
call's breakpoints, how many carry the event inside their CIGAR, and where those alignments put the breakpoints.  This module is
the rule - the regions of a locus (`regions`), the events of a record (`events`), a region's counts, histograms and modes
(`answer`), a locus's payload and columns (`payload`, `columns`) - and the mode's surface for cli.py and the VCF writer (INFO,
COLUMNS, pack, unpack, columns_many).  The readers that apply the rule to a BAM file are seqio.*.signature_many:
bam_signature_kernel on the device, vapor_bam_signature on the host, `answer` over bamio's records."""
from __future__ import annotations

from typing import List, Optional

C = 30                         # minimum clip: the S/H bases at an end of a record that make a clip event
T = 50                         # tolerance: an event counts within T bases of a breakpoint
P = 10000                      # split threshold: breakpoints further apart are two regions
TOL_MAX = 255                  # the widest tolerance a region may ask (the device's histograms are 2 * (2 * 255 + 1) words)
NCAP = (1 << 28) - 1           # the longest operation a BAM record holds: length bounds above it are clamped
EXCLUDE = 0x704                # never counted: unmapped, secondary, QC-fail, duplicate - supplementary records (0x800) count
TYPES = ("DEL", "TANDUP", "INV", "INS")
LCLIP0, RCLIP0, LCLIP1, RCLIP1, GAP, INSOP = 1, 2, 4, 8, 16, 32        # the bits of a region's mask, the order of its six counts
FIELDS = ("w0", "w3", "x0", "x1", "tol", "min_clip", "nmin", "nmax", "mask")     # a region, as every reader takes it
_MASK = {"DEL": RCLIP0 | LCLIP1 | GAP, "TANDUP": LCLIP0 | RCLIP1 | INSOP, "INV": LCLIP0 | RCLIP0 | LCLIP1 | RCLIP1,
         "INS": RCLIP0 | LCLIP1 | INSOP}

INFO = (
    ("VaPoR_SIG_L", "Integer", "1", "Alignments clipped at the left breakpoint (--signatures)"),
    ("VaPoR_SIG_R", "Integer", "1", "Alignments clipped at the right breakpoint (--signatures)"),
    ("VaPoR_SIG_CG", "Integer", "1", "Alignments that carry the event in their CIGAR, a D or N for DEL and an I for INS and TANDUP (--signatures)"),
    ("VaPoR_SIG_N", "Integer", "1", "Signature reads, VaPoR_SIG_CG + max(VaPoR_SIG_L, VaPoR_SIG_R) (--signatures)"),
    ("VaPoR_SIG_POS", "Integer", "1", "Modal left breakpoint of the signature alignments (--signatures)"),
    ("VaPoR_SIG_END", "Integer", "1", "Modal right breakpoint of the signature alignments (--signatures)"),
)
COLUMNS = tuple(i[0] for i in INFO)

# The reader surface (as depth.py's).  ASKED_WITHOUT_CHUNKS: the library refuses a region in its own words, also one no chunk overlaps.
ROW_WIDTH, WINDOW, ZERO, DTYPE = len(FIELDS), (0, 1), (0,) * 10, "int64"
ENTRIES, DEVICE, NATIVE, MANY = ("vapor_bam_signature", "vapor_bam_signature_device"), "bam_signature_device", "signature_native", "signature_many"
LINKED, ASKED_WITHOUT_CHUNKS = False, True

_ADVANCES = (1, 0, 1, 1, 0, 0, 0, 1, 1)      # M I D N S H P = X: moves the reference cursor


def regions(svtype: str, locus, contig_len: int) -> list:
    """The signature regions of a locus on a contig of contig_len bases: a list of FIELDS tuples, none for a type that is not
    measured.  locus = [chrom, s, e] (1-based inclusive) for DEL, TANDUP and INV - the breakpoints are J0 = s - 1 and J1 = e,
    0-based - and (chrom, pos, len) for INS, both breakpoints at pos.  One region when J1 - J0 <= P, else one per breakpoint:
    the second has x0 = x1 = J1 and the bits 0 / 1 for what bits 2 / 3 mean; GAP stays on in the first only, INSOP in neither.
    The window's bounds are clipped to [0, contig_len]."""
    if svtype not in TYPES:
        return []
    if svtype == "INS":
        j0 = j1 = int(locus[1])
        length = int(locus[2])
    else:
        s, e = int(locus[1]), int(locus[2])
        j0, j1, length = s - 1, e, e - s + 1
    mask = _MASK[svtype]
    if mask & (GAP | INSOP):
        nmin, nmax = min(max(C, (length + 1) // 2), NCAP), min(max(2 * length, 0), NCAP)
        if nmin > nmax:                          # (an event of less than C / 2 bases: no operation is both long enough and near its length)
            mask &= ~(GAP | INSOP)
            nmin = nmax = 0
    else:
        nmin = nmax = 0
    n = max(int(contig_len), 0)

    def window(lo, hi):
        a = min(max(lo, 0), n)
        return a, max(min(max(hi, 0), n), a)
    if j1 - j0 <= P:
        w0, w3 = window(j0 - T - 1, j1 + T + 1)
        return [(w0, w3, j0, j1, T, C, nmin, nmax, mask)]
    a0, a3 = window(j0 - T - 1, j0 + T + 1)
    b0, b3 = window(j1 - T - 1, j1 + T + 1)
    first = (a0, a3, j0, j1, T, C, nmin if mask & GAP else 0, nmax if mask & GAP else 0, mask & (LCLIP0 | RCLIP0 | GAP))
    second = (b0, b3, j1, j1, T, C, 0, 0, (mask >> 2) & (LCLIP0 | RCLIP0))
    return [first, second]


def events(pos0: int, ops, min_clip: int = C) -> list:
    """The events of a record at 0-based `pos0` with operations `ops` (uint32, length << 4 | code), in the order LCLIP, the
    operations' GAP and INSOP, RCLIP: ("LCLIP", p), ("GAP", a, n), ("INSOP", a, n), ("RCLIP", q).  The leading clip is read from
    the first two operations, the trailing from the last two (a valid BAM has at most an H and an S at an end); a record of at
    most two operations that are all S or H has neither, and its other operations - none - no event.  A clip event needs
    max(min_clip, 1) clipped bases."""
    ops = ops.tolist() if hasattr(ops, "tolist") else list(ops)
    n_ops = len(ops)
    if not n_ops:
        return []

    def is_clip(o):
        return (o & 15) in (4, 5)
    need = max(int(min_clip), 1)
    all_clip = n_ops <= 2 and all(is_clip(o) for o in ops)
    out = []
    if not all_clip and is_clip(ops[0]):
        lead = (ops[0] >> 4) + ((ops[1] >> 4) if n_ops >= 2 and is_clip(ops[1]) else 0)
        if lead >= need:
            out.append(("LCLIP", int(pos0)))
    cur = int(pos0)
    for o in ops:
        code, n = o & 15, o >> 4
        if code in (2, 3):
            out.append(("GAP", cur, n))
        elif code == 1:
            out.append(("INSOP", cur, n))
        if code <= 8 and _ADVANCES[code]:
            cur += n
    if not all_clip and is_clip(ops[-1]):
        trail = (ops[-1] >> 4) + ((ops[-2] >> 4) if n_ops >= 2 and is_clip(ops[-2]) else 0)
        if trail >= need:
            out.append(("RCLIP", cur))
    return out


def mode_of(hist, tol: int):
    """(offset, count) of a histogram over offsets -tol .. tol: the largest count, among ties the smallest |offset|, then the
    negative offset; (0, 0) for an empty one."""
    best = (0, 0)
    for i, c in enumerate(hist):
        off = i - tol
        if c > best[1] or (c == best[1] and c > 0 and (abs(off), off) < (abs(best[0]), best[0])):
            best = (off, c)
    return best


def answer(records, region):
    """(counts, histograms, modes) of the records over a region (a FIELDS tuple): the six counts in mask-bit order, the two
    histograms over offsets -tol .. tol, and (offset, count) of each.  records: (pos, ops) pairs, pos the 1-based POS - what
    bamio.BamFile.fetch_raw gives; the caller has applied the filter.  A record at or behind w3 is not looked at."""
    w0, w3, x0, x1, tol, min_clip, nmin, nmax, mask = [int(v) for v in region]
    if not 0 <= tol <= TOL_MAX:
        raise ValueError("signature: the tolerance must be between 0 and %d, not %d" % (TOL_MAX, tol))
    counts = [0] * 6
    hist = [[0] * (2 * tol + 1), [0] * (2 * tol + 1)]
    xs = (x0, x1)
    for pos, ops in records:
        p0 = int(pos) - 1
        if p0 >= w3 or w3 <= w0:                 # (an empty window has no records)
            continue
        for ev in events(p0, ops, min_clip):
            if ev[0] in ("LCLIP", "RCLIP"):
                for k in (0, 1):
                    bit = (0 if ev[0] == "LCLIP" else 1) + 2 * k
                    d = ev[1] - xs[k]
                    if (mask >> bit) & 1 and abs(d) <= tol:
                        counts[bit] += 1
                        hist[k][d + tol] += 1
            elif ev[0] == "GAP":
                a, n = ev[1], ev[2]
                if mask & GAP and nmin <= n <= nmax and abs(a - x0) <= tol and abs(a + n - x1) <= tol:
                    counts[4] += 1
                    hist[0][a - x0 + tol] += 1
                    hist[1][a + n - x1 + tol] += 1
            else:
                a, n = ev[1], ev[2]
                if mask & INSOP and nmin <= n <= nmax and x0 - tol <= a <= x1 + tol:
                    counts[5] += 1
                    if abs(a - x0) <= tol:
                        hist[0][a - x0 + tol] += 1
    return counts, hist, (mode_of(hist[0], tol), mode_of(hist[1], tol))


def words(ans) -> list:
    """An answer as the native readers give it: the six counts, then offset and count of each mode."""
    counts, _hist, modes = ans
    return list(counts) + [modes[0][0], modes[0][1], modes[1][0], modes[1][1]]


def statement(records, row, partner=None, min_mapq=0) -> list:
    """The Python statement the readers are held to: a region's words from its records (pos, ops)."""
    return words(answer(records, row))


def locus_regions(svtype: str, locus, length_of) -> list:
    """A locus's regions as the chunk hook sends them: [(contig, FIELDS tuple, None)]; length_of(contig): the contig's length."""
    return [(locus[0], f, None) for f in regions(svtype, locus, length_of(locus[0]))] if svtype in TYPES else []


def merge_words(a, b) -> list:
    """The answers of one region from two files of a per-chromosome pattern: the counts summed, of each mode the better of the
    two by the tie rule (the histograms do not leave the readers)."""
    out = [int(x) + int(y) for x, y in zip(a[:6], b[:6])]
    for k in (6, 8):
        ma, mb = (int(a[k]), int(a[k + 1])), (int(b[k]), int(b[k + 1]))
        better = ma if (-ma[1], abs(ma[0]), ma[0]) <= (-mb[1], abs(mb[0]), mb[0]) else mb
        out += [better[0] if better[1] else 0, better[1]]
    return out


def parse_cigar(text: str) -> list:
    """A CIGAR text as `events`' operations ('*' and '' : none)."""
    from .depth import parse_cigar as _p
    return _p(text)


class Payload(list):
    """[l, r, cg, off0, cnt0, off1, cnt1] with the locus's type and the two 1-based coordinates the offsets are added to."""
    svtype, start, end = "DEL", 0, 0

    def __init__(self, values, svtype="DEL", start=0, end=0):
        super().__init__(int(v) for v in values)
        self.svtype, self.start, self.end = svtype, int(start), int(end)


def payload(svtype: str, locus, regs, answers) -> Optional[Payload]:
    """A locus's payload from its regions and their answers (ten words each, `words`); None for a locus that is not measured.
    l and r are the clip counts at the left and the right breakpoint (for INV the sum of each one's two bits), cg the GAP or
    INSOP count.  An INS has one breakpoint: its two modes are one, the better by the tie rule."""
    if svtype not in TYPES or not regs:
        return None
    a = [int(v) for v in answers[0]]
    if len(regs) == 1:
        l, r, cg = a[0] + a[1], a[2] + a[3], a[4] + a[5]
        m0, m1 = (a[6], a[7]), (a[8], a[9])
    else:
        b = [int(v) for v in answers[1]]
        l, r, cg = a[0] + a[1], b[0] + b[1], a[4]
        m0, m1 = (a[6], a[7]), (b[6], b[7])
    if svtype == "INS":
        m0 = m1 = min(m0, m1, key=lambda m: (-m[1], abs(m[0]), m[0]))
        s = e = int(locus[1])
    else:
        s, e = int(locus[1]), int(locus[2])
    return Payload([l, r, cg, m0[0], m0[1], m1[0], m1[1]], svtype, s, e)


locus_payload = payload              # (of locus_regions' list only its length is read)


def columns(p) -> List[str]:
    """The six columns of a payload as text: L, R, CG, N = CG + max(L, R) (a split molecule shows one clip on each side: max
    counts it once), POS = start + off0 and END = end + off1, '.' without a mode."""
    if p is None:
        return ["."] * 6
    l, r, cg, off0, cnt0, off1, cnt1 = [int(x) for x in p[:7]]
    return [str(l), str(r), str(cg), str(cg + max(l, r)), str(p.start + off0) if cnt0 else ".", str(p.end + off1) if cnt1 else "."]


def pack(p) -> List[float]:
    """The payload as floats for the gather across ranks: the seven integers, the type as its index in TYPES, the two
    coordinates (all below 2^53: exact); nothing for a locus without one."""
    if p is None:
        return []
    return [float(v) for v in p] + [float(TYPES.index(p.svtype)), float(p.start), float(p.end)]


def unpack(flat) -> Optional[Payload]:
    if flat is None or len(flat) == 0:
        return None
    return Payload(flat[:7], TYPES[int(flat[7])], flat[8], flat[9])


def columns_many(payloads) -> List[List[str]]:
    return [columns(p) for p in payloads]

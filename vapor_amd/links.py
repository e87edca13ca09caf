"""`vapor bed | vcf --links`: split reads joined through their SA tags - of the alignments clipped at a call's
breakpoint, how many name, in their SA tag, a piece at the call's other breakpoint with the strand the event gives it, how many
are split but go elsewhere, and where the linked pieces put the other breakpoint.  This module is the rule - the SA entries of a
record (`parse_sa`), the regions of a locus (`regions`), a region's counts, histogram and mode (`answer`), a locus's payload and
columns (`payload`, `columns`) - and the mode's surface for cli.py and the VCF writer (INFO, COLUMNS, pack, unpack,
columns_many).  The clip events are signature.events: they are not stated a second time.  The readers that apply the rule to a
BAM file are seqio.*.links_many: bam_link_kernel on the device, vapor_bam_links on the host, `answer` over bamio's records."""
from __future__ import annotations

from typing import List, Optional

from .signature import EXCLUDE, TOL_MAX, events, mode_of  # noqa: F401  (EXCLUDE: what the readers never count)

C = 30                         # minimum clip, as signature.C
T = 50                         # tolerance at both ends of a link, as signature.T
POS_MAX = (1 << 31) - 1        # the largest pos of an entry
OP_MAX = (1 << 28) - 1         # the longest operation of an entry's CIGAR
LCLIP, RCLIP = 0, 1            # ev
END_A, END_B = 0, 1            # pend
SAME, OTHER = 0, 1             # rel
FIELDS = ("w0", "w3", "x", "y", "tol", "min_clip", "ev", "pend", "rel")     # a region's integers; its contig and partner go beside
TYPES = ("DEL", "TANDUP", "INV", "BND")

INFO = (
    ("VaPoR_LNK_L", "Integer", "1", "Alignments clipped at the left breakpoint whose SA tag names a piece at the right one (--links)"),
    ("VaPoR_LNK_R", "Integer", "1", "Alignments clipped at the right breakpoint whose SA tag names a piece at the left one (--links)"),
    ("VaPoR_LNK_N", "Integer", "1", "Linked split reads, max(VaPoR_LNK_L, VaPoR_LNK_R) (--links)"),
    ("VaPoR_LNK_OL", "Integer", "1", "Alignments clipped at the left breakpoint whose SA entries all lie elsewhere (--links)"),
    ("VaPoR_LNK_OR", "Integer", "1", "Alignments clipped at the right breakpoint whose SA entries all lie elsewhere (--links)"),
    ("VaPoR_LNK_POS", "Integer", "1", "Modal first coordinate named by the SA tags of the right side's linked alignments (--links)"),
    ("VaPoR_LNK_END", "Integer", "1", "Modal second coordinate named by the SA tags of the left side's linked alignments (--links)"),
)
COLUMNS = tuple(i[0] for i in INFO)

# The reader surface (as depth.py's).  A row is FIELDS, then offset and length of the partner contig's name in the call's blob of
# names.  LINKED: a region has a partner contig, and its records carry FLAG and the SA value (bamio's fetch_links, sa_of_sam of a
# SAM line).  ASKED_WITHOUT_CHUNKS: the library refuses a region in its own words, also one no chunk overlaps.
ROW_WIDTH, WINDOW, ZERO, DTYPE = len(FIELDS) + 2, (0, 1), (0,) * 5, "int64"
ENTRIES, DEVICE, NATIVE, MANY = ("vapor_bam_links", "vapor_bam_links_device"), "bam_links_device", "links_native", "links_many"
LINKED = ASKED_WITHOUT_CHUNKS = True

_OPS = b"MIDNSHP=X"
_ADVANCE = (1, 0, 1, 1, 0, 0, 0, 1, 1)


def _number(b: bytes, max_digits: int):
    if not 1 <= len(b) <= max_digits or not all(48 <= c <= 57 for c in b):
        return None
    return int(b)


def parse_piece(piece: bytes):
    """(rname, a, b, strand, mapq) of one piece of an SA value - rname as bytes, [a, b) 0-based half-open, strand '+' or '-' -
    or None when the piece is not well-formed: it must be, as bytes and in full, rname,pos,strand,CIGAR,mapQ,NM with a
    non-empty rname free of ',' and ';', pos of 1..10 digits in 1 .. 2^31 - 1, strand + or -, a CIGAR of one or more operations
    of 1..9 digits (at most 2^28 - 1) and a letter of MIDNSHP=X, mapQ of 1..3 digits at most 255, NM of one or more digits."""
    if b";" in piece:
        return None
    f = piece.split(b",")
    if len(f) != 6 or not f[0]:
        return None
    pos, mapq = _number(f[1], 10), _number(f[4], 3)
    if pos is None or not 1 <= pos <= POS_MAX or mapq is None or mapq > 255 or f[2] not in (b"+", b"-"):
        return None
    if not f[5] or not all(48 <= c <= 57 for c in f[5]):
        return None
    cg = f[3]
    if not cg:
        return None
    span, i, n = 0, 0, len(cg)
    while i < n:
        j = i
        while j < n and 48 <= cg[j] <= 57:
            j += 1
        if j == i or j - i > 9 or j >= n:
            return None
        code = _OPS.find(cg[j:j + 1])
        length = int(cg[i:j])
        if code < 0 or length > OP_MAX:
            return None
        if _ADVANCE[code]:
            span += length
        i = j + 1
    return f[0], pos - 1, pos - 1 + span, f[2].decode(), mapq


def parse_sa(value, min_mapq: int = 0) -> list:
    """The entries (rname, a, b, strand) of an SA value (bytes: what stands before the NUL; None: no entries) in text order: the
    value cut at every ';', empty pieces dropped, a last piece without ';' a piece; a piece that is not well-formed
    (parse_piece) and one with mapQ below min_mapq are ignored."""
    if not value:
        return []
    out = []
    for piece in bytes(value).split(b";"):
        if not piece:
            continue
        e = parse_piece(piece)
        if e is not None and e[4] >= min_mapq:
            out.append(e[:4])
    return out


def sa_of_sam(fields) -> Optional[bytes]:
    """The SA value among the optional fields of a SAM line (`TAG:TYPE:VALUE` strings): the first field named SA, when its type
    is Z; None otherwise."""
    for f in fields:
        if f[:3] == "SA:":
            return f[5:].encode("latin-1") if f[3:5] == "Z:" else None
    return None


def _window(x: int, n: int):
    lo, hi = x - T - 1, x + T + 1
    a = min(max(lo, 0), n)
    return a, max(min(max(hi, 0), n), a)


def regions(svtype: str, locus, length_of) -> tuple:
    """(left, right): the link regions of a locus's two sides, each a list of (contig, FIELDS tuple, partner contig); two empty
    lists for a locus that is not measured.  locus = [chrom, s, e] (1-based inclusive) for DEL, TANDUP and INV - J0 = s - 1 and
    J1 = e, 0-based - and the scored view [A, p, B, q, CT, ..] for BND (CT '3to5' or '3to3'; cli.bnd_view has mirrored a 5to3
    record).  length_of(contig): the contig's length, to which every window [x - T - 1, x + T + 1) is clipped.  Every question
    is one region (the table of loci)."""
    def reg(c, x, ev, pc, y, pend, rel):
        w0, w3 = _window(x, max(int(length_of(c)), 0))
        return (c, (w0, w3, x, y, T, C, ev, pend, rel), pc)
    if svtype in ("DEL", "TANDUP", "INV"):
        c, s, e = locus[0], int(locus[1]), int(locus[2])
        j0, j1 = s - 1, e
        if svtype == "DEL":
            return [reg(c, j0, RCLIP, c, j1, END_A, SAME)], [reg(c, j1, LCLIP, c, j0, END_B, SAME)]
        if svtype == "TANDUP":
            return [reg(c, j0, LCLIP, c, j1, END_B, SAME)], [reg(c, j1, RCLIP, c, j0, END_A, SAME)]
        return ([reg(c, j0, RCLIP, c, j1, END_B, OTHER), reg(c, j0, LCLIP, c, j1, END_A, OTHER)],
                [reg(c, j1, RCLIP, c, j0, END_B, OTHER), reg(c, j1, LCLIP, c, j0, END_A, OTHER)])
    if svtype == "BND" and len(locus) >= 5:
        a, p, b, q, ct = locus[0], int(locus[1]), locus[2], int(locus[3]), locus[4]
        if ct == "3to5":
            return [reg(a, p, RCLIP, b, q - 1, END_A, SAME)], [reg(b, q - 1, LCLIP, a, p, END_B, SAME)]
        if ct == "3to3":
            return [reg(a, p, RCLIP, b, q, END_B, OTHER)], [reg(b, q, RCLIP, a, p, END_B, OTHER)]
    return [], []


def region_ok(fields, partner) -> bool:
    """Whether a region is a question the readers answer (vapor_readplan.h link_region_ok)."""
    w0, w3, _x, _y, tol, _mc, ev, pend, rel = [int(v) for v in fields]
    return (0 <= w0 <= w3 < (1 << 31) and 0 <= tol <= TOL_MAX and ev in (0, 1) and pend in (0, 1) and rel in (0, 1) and len(partner) > 0)


def answer(records, fields, partner, min_mapq: int = 0):
    """(n_clip, n_split, n_link, histogram, mode) of the records over a region (FIELDS) whose partner contig is `partner` (str or
    bytes).  records: (pos, ops, flag, sa) - the 1-based POS, the operations, FLAG and the SA value as bytes or None; the caller
    has applied the filter.  A record at or behind w3 is not looked at.  min_mapq: the cut on the entries' mapQ."""
    w0, w3, x, y, tol, min_clip, ev, pend, rel = [int(v) for v in fields]
    pb = partner.encode("latin-1") if isinstance(partner, str) else bytes(partner)
    if not region_ok(fields, pb):
        raise ValueError("links: not a region the readers answer: %r, partner %r" % (tuple(fields), partner))
    want = "RCLIP" if ev == RCLIP else "LCLIP"
    n_clip = n_split = n_link = 0
    hist = [0] * (2 * tol + 1)
    for pos, ops, flag, sa in records:
        p0 = int(pos) - 1
        if p0 >= w3 or w3 <= w0:                 # (an empty window has no records)
            continue
        if not any(e[0] == want and abs(e[1] - x) <= tol for e in events(p0, ops, min_clip)):
            continue
        n_clip += 1
        entries = parse_sa(sa, min_mapq)
        if not entries:
            continue
        n_split += 1
        minus = bool(int(flag) & 0x10)
        for rname, a, b, strand in entries:
            c = b if pend == END_B else a
            if rname == pb and ((strand == "-") != minus) == bool(rel) and abs(c - y) <= tol:
                n_link += 1
                hist[c - y + tol] += 1
                break
    return n_clip, n_split, n_link, hist, mode_of(hist, tol)


def words(ans) -> list:
    """An answer as the native readers give it: n_clip, n_split, n_link, then offset and count of the mode."""
    return [ans[0], ans[1], ans[2], ans[4][0], ans[4][1]]


def statement(records, row, partner, min_mapq=0) -> list:
    """The Python statement the readers are held to: a region's words from its records (pos, ops, flag, sa); row: FIELDS, and
    whatever a reader keeps behind them."""
    return words(answer(records, row[:len(FIELDS)], partner, min_mapq))


def locus_regions(svtype: str, locus, length_of) -> list:
    """A locus's regions as the chunk hook sends them: `regions`' left side, then its right - as many each."""
    left, right = regions(svtype, locus, length_of)
    return left + right


def locus_payload(svtype: str, locus, regs, answers) -> Optional["Payload"]:
    """The locus's Payload from locus_regions' list and the regions' words: the first half is the left side's."""
    half = len(regs) // 2
    return payload(svtype, locus, answers[:half], answers[half:])


def merge_words(a, b) -> list:
    """The answers of one region from two files of a per-chromosome pattern, or of a side's two regions: the counts summed, of
    the modes the better by the tie rule."""
    out = [int(x) + int(y) for x, y in zip(a[:3], b[:3])]
    ma, mb = (int(a[3]), int(a[4])), (int(b[3]), int(b[4]))
    better = ma if (-ma[1], abs(ma[0]), ma[0]) <= (-mb[1], abs(mb[0]), mb[0]) else mb
    return out + [better[0] if better[1] else 0, better[1]]


class Payload(list):
    """[link_l, split_l, link_r, split_r, off_l, cnt_l, off_r, cnt_r] with the row's two 1-based coordinates: start and end of a
    DEL, TANDUP or INV, p and q of a breakend."""
    start, end = 0, 0

    def __init__(self, values, start=0, end=0):
        super().__init__(int(v) for v in values)
        self.start, self.end = int(start), int(end)


def payload(svtype: str, locus, left, right) -> Optional[Payload]:
    """A locus's payload from the answers (five words each, `words`) of its left and right regions; None for a locus without
    regions.  A side's counts are summed over its regions and of their modes the better is kept."""
    if svtype not in TYPES or not left or not right:
        return None
    zero = [0, 0, 0, 0, 0]
    l, r = zero, zero
    for a in left:
        l = merge_words(l, a)
    for a in right:
        r = merge_words(r, a)
    start, end = (int(locus[1]), int(locus[3])) if svtype == "BND" else (int(locus[1]), int(locus[2]))
    return Payload([l[2], l[1], r[2], r[1], l[3], l[4], r[3], r[4]], start, end)


def columns(p) -> List[str]:
    """The seven columns of a payload as text: L, R, N = max(L, R) (a split molecule shows once on each side), OL and OR =
    n_split - n_link, POS = start + the right side's offset and END = end + the left side's, '.' without a mode."""
    if p is None:
        return ["."] * 7
    ll, sl, lr, sr, off_l, cnt_l, off_r, cnt_r = [int(v) for v in p[:8]]
    return [str(ll), str(lr), str(max(ll, lr)), str(sl - ll), str(sr - lr),
            str(p.start + off_r) if cnt_r else ".", str(p.end + off_l) if cnt_l else "."]


def pack(p) -> List[float]:
    """The payload as floats for the gather across ranks: the eight integers and the two coordinates (all below 2^53: exact);
    nothing for a locus without one."""
    if p is None:
        return []
    return [float(v) for v in p] + [float(p.start), float(p.end)]


def unpack(flat) -> Optional[Payload]:
    if flat is None or len(flat) == 0:
        return None
    return Payload(flat[:8], flat[8], flat[9])


def columns_many(payloads) -> List[List[str]]:
    return [columns(p) for p in payloads]

"""`vapor bed | vcf --support`: alt and ref alignments per call - how many records carry the event, how many run
straight through a breakpoint as the reference allele does, and the allele fraction and genotype the two numbers give.  This
module is the rule - the regions of a locus (`regions`), a record's facts (`facts`), a region's seven words (`answer`), the
genotype of two counts (`genotype`), a locus's payload and columns (`payload`, `columns`) - and the mode's surface for cli.py and
the VCF writer (INFO, COLUMNS, pack, unpack, columns_many).  The events, the mask bits 0 to 5 and the length bounds are
signature.py's.  The readers that apply the rule to a BAM file are seqio.*.support_many: bam_support_kernel on
the device, vapor_bam_support on the host, `answer` over bamio's records."""
from __future__ import annotations

import math
from typing import List, Optional

from . import signature
from .signature import C, EXCLUDE, GAP, INSOP, P, T, TOL_MAX, TYPES, parse_cigar  # noqa: F401  (the mode's readers name them here)

F = T + 1                      # flank: a reference alignment reaches F bases to either side of a breakpoint - the window's edges
G = C                          # the shortest D, N or I near a breakpoint that makes a record no reference alignment
FLANK_MAX = 65535              # the widest flank a region may ask
REF0, REF1 = 64, 128           # mask bits 6 and 7: reference support is asked at x0 / at x1
ERR = 0.05                     # the genotype model's error rate: an alignment of the other allele
FIELDS = signature.FIELDS + ("flank", "gmin")      # a region, as every reader takes it
WORDS = ("alt_cg", "alt_l", "alt_r", "ref_0", "ref_1", "cov_0", "cov_1")     # its answer

INFO = (
    ("VaPoR_SUP_ALT", "Integer", "1", "Alignments that carry the event, in their CIGAR or as a clip at a breakpoint (--support)"),
    ("VaPoR_SUP_REF", "Integer", "1", "Alignments that run through a breakpoint as the reference does, max of left and right (--support)"),
    ("VaPoR_SUP_REFL", "Integer", "1", "Alignments that run through the left breakpoint as the reference does (--support)"),
    ("VaPoR_SUP_REFR", "Integer", "1", "Alignments that run through the right breakpoint as the reference does (--support)"),
    ("VaPoR_SUP_COVL", "Integer", "1", "Alignments that cover the base at the left breakpoint (--support)"),
    ("VaPoR_SUP_COVR", "Integer", "1", "Alignments that cover the base at the right breakpoint (--support)"),
    ("VaPoR_SUP_VAF", "Float", "1", "Allele fraction of the alignments, VaPoR_SUP_ALT / (VaPoR_SUP_ALT + VaPoR_SUP_REF) (--support)"),
    ("VaPoR_SUP_GT", "String", "1", "Genotype of the alignments: the likeliest of 0/0, 0/1 and 1/1 at an error rate of 0.05 (--support)"),
    ("VaPoR_SUP_GQ", "Integer", "1", "Quality of VaPoR_SUP_GT: ten times the log10 likelihood ratio to the second genotype, at most 99 (--support)"),
)
COLUMNS = tuple(i[0] for i in INFO)

# The reader surface (as depth.py's).  ASKED_WITHOUT_CHUNKS: the library refuses a region in its own words, also one no chunk overlaps.
ROW_WIDTH, WINDOW, ZERO, DTYPE = len(FIELDS), (0, 1), (0,) * 7, "int64"
ENTRIES, DEVICE, NATIVE, MANY = ("vapor_bam_support", "vapor_bam_support_device"), "bam_support_device", "support_native", "support_many"
LINKED, ASKED_WITHOUT_CHUNKS = False, True


def regions(svtype: str, locus, contig_len: int) -> list:
    """The support regions of a locus: signature.regions' (the same windows, the same split at P) with F and G behind each and
    the bits that ask for reference support.  One region: both bits.  Two: bit 6 in each - the first's x1 lies outside its walk,
    the second has x0 = x1 = J1 and its target-0 words are the right breakpoint's."""
    regs = signature.regions(svtype, locus, contig_len)
    if len(regs) == 1:
        return [regs[0][:8] + (regs[0][8] | REF0 | REF1, F, G)]
    return [r[:8] + (r[8] | REF0, F, G) for r in regs]


def region_ok(region) -> bool:
    """Whether the fields are a question the readers answer (vapor_readplan.h sup_region_ok, without the contig)."""
    w0, w3, _x0, _x1, tol, _mc, nmin, nmax, _mask, flank, gmin = [int(v) for v in region]
    return 0 <= w0 <= w3 < (1 << 31) and 0 <= tol <= TOL_MAX and nmin <= nmax and 1 <= flank <= FLANK_MAX and gmin >= 1


def facts(pos0: int, ops, region) -> Optional[dict]:
    """The facts of one record at 0-based `pos0` over a region: cg, clip (two), blocked (two), span (two), cov (two) and its
    reference end q.  None for a record without operations."""
    _w0, _w3, x0, x1, tol, min_clip, nmin, nmax, mask, flank, gmin = [int(v) for v in region]
    ops = ops.tolist() if hasattr(ops, "tolist") else list(ops)
    if not ops:
        return None
    xs = (x0, x1)
    cg = False
    clip = [False, False]
    blocked = [False, False]
    q = int(pos0)
    for ev in signature.events(pos0, ops, min_clip):
        if ev[0] in ("LCLIP", "RCLIP"):
            for k in (0, 1):
                bit = (0 if ev[0] == "LCLIP" else 1) + 2 * k
                if (mask >> bit) & 1 and abs(ev[1] - xs[k]) <= tol:
                    clip[k] = True
            continue
        a, n = ev[1], ev[2]
        if ev[0] == "GAP":
            if mask & GAP and nmin <= n <= nmax and abs(a - x0) <= tol and abs(a + n - x1) <= tol:
                cg = True
            for k in (0, 1):
                if n >= gmin and a < xs[k] + flank and a + n > xs[k] - flank:
                    blocked[k] = True
        else:
            if mask & INSOP and nmin <= n <= nmax and x0 - tol <= a <= x1 + tol:
                cg = True
            for k in (0, 1):
                if n >= gmin and xs[k] - flank <= a <= xs[k] + flank:
                    blocked[k] = True
    for o in ops:
        if (o & 15) in (0, 2, 3, 7, 8):
            q += o >> 4
    span = [pos0 <= xs[k] - flank and q >= xs[k] + flank and not blocked[k] for k in (0, 1)]
    cov = [pos0 <= xs[k] < q for k in (0, 1)]
    return {"cg": cg, "clip": clip, "blocked": blocked, "span": span, "cov": cov, "q": q}


def answer(records, region) -> list:
    """The seven words (WORDS) of the records over a region (a FIELDS tuple).  records: (pos, ops) pairs, pos the 1-based POS -
    what bamio.BamFile.fetch_raw gives; the caller has applied the filter.  A record at or behind w3 is not looked at."""
    if not region_ok(region):
        raise ValueError("support: not a region the readers answer: %r" % (tuple(int(v) for v in region),))
    w0, w3, mask = int(region[0]), int(region[1]), int(region[8])
    out = [0] * 7
    for pos, ops in records:
        p0 = int(pos) - 1
        if p0 >= w3 or w3 <= w0:                 # (an empty window has no records)
            continue
        f = facts(p0, ops, region)
        if f is None:
            continue
        cg = f["cg"]
        out[0] += cg
        for k in (0, 1):
            out[1 + k] += f["clip"][k] and not cg
            out[3 + k] += bool(mask & (REF0, REF1)[k]) and f["span"][k] and not cg and not f["clip"][k]
            out[5 + k] += f["cov"][k]
    return [int(v) for v in out]


def statement(records, row, partner=None, min_mapq=0) -> list:
    """The Python statement the readers are held to: a region's words from its records (pos, ops)."""
    return answer(records, row)


def locus_regions(svtype: str, locus, length_of) -> list:
    """A locus's regions as the chunk hook sends them: [(contig, FIELDS tuple, None)]; length_of(contig): the contig's length."""
    return [(locus[0], f, None) for f in regions(svtype, locus, length_of(locus[0]))] if svtype in TYPES else []


def merge_words(a, b) -> list:
    """The answers of one region from two files of a per-chromosome pattern: summed."""
    return [int(x) + int(y) for x, y in zip(a, b)]


def genotype(alt: int, ref: int):
    """(GT, GQ) of ALT alt and REF ref alignments, (None, None) without any: the largest of the log10 likelihoods
    L0 = ALT log10(e) + REF log10(1 - e), L1 = (ALT + REF) log10(0.5), L2 = ALT log10(1 - e) + REF log10(e), ties to fewer alt
    alleles; GQ = min(99, floor(10 (best - second)))."""
    alt, ref = int(alt), int(ref)
    if alt + ref == 0:
        return None, None
    ls = (alt * math.log10(ERR) + ref * math.log10(1 - ERR), (alt + ref) * math.log10(0.5), alt * math.log10(1 - ERR) + ref * math.log10(ERR))
    best = max(range(3), key=lambda i: (ls[i], -i))
    second = max(ls[i] for i in range(3) if i != best)
    return ("0/0", "0/1", "1/1")[best], min(99, int(math.floor(10 * (ls[best] - second))))


class Payload(list):
    """[alt_cg, alt_l, alt_r, ref_l, ref_r, cov_l, cov_r] with the locus's type and its two 1-based coordinates."""
    svtype, start, end = "DEL", 0, 0

    def __init__(self, values, svtype="DEL", start=0, end=0):
        super().__init__(int(v) for v in values)
        self.svtype, self.start, self.end = svtype, int(start), int(end)


def payload(svtype: str, locus, regs, answers) -> Optional[Payload]:
    """A locus's payload from its regions and their answers (seven words each); None for a locus that is not measured.  One
    region: its words.  Two: the left breakpoint's from the first, the right one's from the second's target 0 (the first's
    cov_1 and every word of the second's target 1 are ignored)."""
    if svtype not in TYPES or not regs:
        return None
    a = [int(v) for v in answers[0]]
    if len(regs) == 1:
        vals = a
    else:
        b = [int(v) for v in answers[1]]
        vals = [a[0], a[1], b[1], a[3], b[3], a[5], b[5]]
    if svtype == "INS":
        s = e = int(locus[1])
    else:
        s, e = int(locus[1]), int(locus[2])
    return Payload(vals, svtype, s, e)


locus_payload = payload              # (of locus_regions' list only its length is read)


def columns(p) -> List[str]:
    """The nine columns of a payload as text.  ALT = alt_cg + max(alt_l, alt_r) and REF = max(ref_l, ref_r): a split molecule,
    and a reference molecule that spans both breakpoints, counts once.  VAF, GT and GQ are '.' without an alignment, and for a
    TANDUP always: the reads of the duplicated allele cross both outer breakpoints contiguously."""
    if p is None:
        return ["."] * 9
    cg, al, ar, rl, rr, cl, cr = [int(x) for x in p[:7]]
    alt, ref = cg + max(al, ar), max(rl, rr)
    gt, gq = genotype(alt, ref) if p.svtype != "TANDUP" else (None, None)
    return [str(alt), str(ref), str(rl), str(rr), str(cl), str(cr), "%.3f" % (alt / (alt + ref)) if gt is not None else ".",
            gt if gt is not None else ".", str(gq) if gt is not None else "."]


def pack(p) -> List[float]:
    """The payload as floats for the gather across ranks, as signature.pack packs its own: the seven integers, the type as its
    index in TYPES, the two coordinates (all below 2^53: exact); nothing for a locus without one."""
    if p is None:
        return []
    return [float(v) for v in p] + [float(TYPES.index(p.svtype)), float(p.start), float(p.end)]


def unpack(flat) -> Optional[Payload]:
    if flat is None or len(flat) == 0:
        return None
    return Payload(flat[:7], TYPES[int(flat[7])], flat[8], flat[9])


def columns_many(payloads) -> List[List[str]]:
    return [columns(p) for p in payloads]

"""`vapor bed | vcf --realign`: every read of a locus aligned to the reference allele and to the alt allele, and
the allele it fits better.  This module is the rule - the edit distance of a read against an allele inside a band, start anchored
at the window start, both ends free (`statement`, the Python statement the kernel is held to), a read's vote (`votes`), a locus's
payload and columns (`payload`, `columns`) - and the mode's surface for cli.py and the VCF writer (INFO, COLUMNS, pack, unpack,
columns_many).  The device computes the distances (realign_kernel through Engine.realign; pipeline.realign_requests makes the
call); there is no other route.  The genotype of the two counts is support.genotype's, so that VaPoR_RA_GT and VaPoR_SUP_GT are
comparable."""
from __future__ import annotations

import collections
from typing import List, Optional

import numpy as np

from . import support

BAND = 256                     # the band of the command line: a cell (i, j) exists iff |i - j| <= BAND
MAX_BAND = 512                 # the widest band the kernel takes (VAPOR_MAX_BAND)
MARGIN = 10                    # a read votes when its two distances differ by at least this (the smallest event the drivers take is
                               # 50 bp, whose expected difference is about the event's length): a rule, not a tolerance

class Options(collections.namedtuple("Options", "trace polish junction revote")):
    """What a `--realign` run asks beside the votes, the one place that spells the four: `trace` (`--realign-out`),
    `polish` (`--realign-polish`, 4.25), `junction` (`--realign-junction`, 4.26) and `revote` (`--realign-revote`, 4.27); the last
    two read the polished allele and need `polish`.  A flag beside `trace` names the section of its module (polish.SECTION, ..)
    and the attribute of the Payload its object rides on."""
    __slots__ = ()

    def __new__(cls, trace=False, polish=False, junction=False, revote=False):
        self = super().__new__(cls, bool(trace), bool(polish), bool(junction), bool(revote))
        if (self.junction or self.revote) and not self.polish:
            raise ValueError("realign: junction and revote need polish")
        return self


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


# ---- `--realign-out`: the alignment behind d ----
OPS = "=XID"                   # the op codes of a run word (len << 2 | op), as vapor_realign_trace writes them
FIRST_CAP_RUNS = 64            # runs a pair of the first Engine.realign_trace call of a batch; an overflow is asked again at n + m + 1


def trace_statement(read, allele, off2: int, band: int):
    """(d, i_end, j_end, runs) of the pair: d as `statement` has it and the alignment 4.24's rule picks.  End cell: of the
    existing cells of the last row and of the last column whose D equals d, the one with the largest i, among those the one
    with the largest j.  From there back to (0, 0), at every cell: the diagonal predecessor if it exists and
    D[i-1][j-1] + sub == D[i][j] ('=' where the symbols match, 'X' where not), otherwise the vertical one if it exists and
    D[i-1][j] + 1 == D[i][j] ('I'), otherwise the horizontal one ('D'); row 0 is all horizontal.  runs: the path reversed and
    run-length encoded, [(length, op)]; the n - i_end read symbols behind the end cell are soft-clipped and are no run.
    `statement`'s rows with one byte kept per slot and row (the move out of that cell), so 65 535 rows fit."""
    band, off2 = int(band), int(off2)
    if not 1 <= band <= MAX_BAND:
        raise ValueError("realign: band %d outside 1 .. %d" % (band, MAX_BAND))
    if not 0 <= off2 <= len(allele):
        raise ValueError("realign: off2 %d outside 0 .. %d" % (off2, len(allele)))
    a = _bases(read, _NEVER_A)
    b = _bases(allele, _NEVER_B)[off2:]
    n, m, w = len(a), len(b), 2 * band + 1
    c = np.arange(w, dtype=np.int64)
    bpad = np.full(n + m + 2 * w + 2, _NEVER_B, dtype=np.int64)
    bpad[band:band + m] = b
    j = c - band
    row = np.where((j >= 0) & (j <= m), j, _BIG)
    col = m + band
    moves = np.zeros((n + 1, w), dtype=np.uint8)
    last_col = np.full(n + 1, _BIG, dtype=np.int64)                  # D[i][m], _BIG where the cell does not exist
    if 0 <= col < w:
        last_col[0] = row[col]
    for i in range(1, n + 1):
        j = c + (i - band)
        sub = (bpad[i - 1:i - 1 + w] != a[i - 1]).astype(np.int64)
        diag = row + sub
        vert = np.append(row[1:], _BIG) + 1
        t = np.where((j >= 0) & (j <= m), np.minimum(diag, vert), _BIG)
        row = np.minimum(np.minimum.accumulate(t - c) + c, _BIG)
        moves[i] = np.where(row == diag, sub, np.where(row == vert, 2, 3))
        s = col - i
        if 0 <= s < w:
            last_col[i] = row[s]
    jn = c + (n - band)
    last_row = np.where((jn >= 0) & (jn <= m), row, _BIG)            # D[n][j] at slot j - n + band
    d = int(min(last_row.min(), last_col.min()))
    on_row = np.nonzero(last_row == d)[0]
    if len(on_row):
        i_end, j_end = n, int(jn[on_row[-1]])
    else:
        i_end, j_end = int(np.nonzero(last_col == d)[0][-1]), m
    i, j, runs = i_end, j_end, []

    def step(op):
        if runs and runs[-1][1] == op:
            runs[-1][0] += 1
        else:
            runs.append([1, op])
    while i > 0:
        mv = int(moves[i, j - i + band])
        step(OPS[mv])
        if mv < 2:
            i, j = i - 1, j - 1
        elif mv == 2:
            i -= 1
        else:
            j -= 1
    if j > 0:
        if runs and runs[-1][1] == "D":
            runs[-1][0] += j
        else:
            runs.append([j, "D"])
    return d, i_end, j_end, [(k, op) for k, op in reversed(runs)]


def runs_of(head, words):
    """[(length, op)] of a pair from its head row and its row of run words (Engine.realign_trace): the last n_runs words."""
    k = int(head[4])
    return [(int(v) >> 2, OPS[int(v) & 3]) for v in words[len(words) - k:]] if k else []


def fold_leading_d(runs):
    """(lead, rest): a leading 'D' run's length - the read starts that far behind the allele's start, which a SAM record says
    with POS - and the runs behind it; (0, runs) without one."""
    if runs and runs[0][1] == "D":
        return int(runs[0][0]), list(runs[1:])
    return 0, list(runs)


def cigar_text(runs, clip: int = 0) -> str:
    """The runs as CIGAR text with a trailing soft clip of `clip` read symbols; '*' for nothing at all."""
    return ("".join("%d%s" % (k, op) for k, op in runs) + ("%dS" % clip if clip else "")) or "*"


def aligned(runs) -> bool:
    """Whether a trace holds an '=' or 'X' run: a read without one is not written."""
    return any(op in "=X" for _k, op in runs)


def fits_alt(diff: int) -> bool:
    """The allele a read's alignment is shown on: an ALT voter against alt, a REF voter against ref, a no-call against the
    smaller distance, a tie against ref - alt iff d_ref - d_alt > 0."""
    return int(diff) > 0


def vote_text(diff: int) -> str:
    return "ALT" if diff >= MARGIN else "REF" if diff <= -MARGIN else "NC"


class Traces:
    """What `--realign-out` writes of a locus: its two alleles as text and, per read in request order, (text, miss_bp, d_ref,
    d_alt, i_end, j_end, runs) - the alignment against the allele the read fits (fits_alt of d_ref - d_alt).  Rides on the
    locus's Payload as `.traces`, on the rank that scored it; pack / unpack never see it."""
    __slots__ = ("ref", "alt", "reads")

    def __init__(self, ref, alt, reads):
        self.ref, self.alt, self.reads = str(ref), str(alt), list(reads)


def sam_record(key: str, index: int, read) -> Optional[str]:
    """The SAM line of read `index` of locus `key`; None for a read whose trace holds no '=' or 'X'."""
    text, miss, d_ref, d_alt, i_end, _j_end, runs = read
    if not aligned(runs):
        return None
    diff = int(d_ref) - int(d_alt)
    on_alt = fits_alt(diff)
    lead, rest = fold_leading_d(runs)
    fields = ["%s/%d" % (key, index), "0", "%s|%s" % (key, "ALT" if on_alt else "REF"), str(int(miss) + 1 + lead), "255",
              cigar_text(rest, len(text) - int(i_end)), "*", "0", "0", str(text), "*", "NM:i:%d" % (d_alt if on_alt else d_ref),
              "rd:i:%d" % d_ref, "ad:i:%d" % d_alt, "vt:Z:%s" % vote_text(diff)]
    return "\t".join(fields)


def numbered(spool):
    """The (key, value) entries of a writer's spool {job index: (key, value)} in job order, a repeated key with #2, #3, .."""
    seen = {}
    for order in sorted(spool):
        key, value = spool[order]
        seen[key] = seen.get(key, 0) + 1
        yield (key if seen[key] == 1 else "%s#%d" % (key, seen[key])), value


class TraceWriter:
    """The sink of `--realign-out PREFIX`: takes the loci a rank scores from any chunk thread, under a lock, and at close writes
    PREFIX.fa and PREFIX.sam (PREFIX.rank<k>.* on rank k of several) in job order, so that the files depend neither on the
    threads nor on the chunking.  PREFIX.fa: per locus with a payload `>KEY|REF` and `>KEY|ALT`, the whole allele on one line,
    KEY the job's key as the table spells it, a repeated key with #2, #3, ..  PREFIX.sam: `@HD VN:1.6 SO:unknown`, one @SQ per
    FASTA entry in that order, then the records (sam_record).  A locus without a payload writes nothing."""

    def __init__(self, prefix: str, rank: int = 0, world: int = 1):
        import threading
        self.stem = prefix if world <= 1 else "%s.rank%d" % (prefix, rank)
        self._lock = threading.Lock()
        self._spool = {}

    def take(self, order: int, key: str, payload) -> None:
        if payload is None or payload.traces is None:
            return
        with self._lock:
            self._spool[int(order)] = (key, payload.traces)

    def close(self):
        names, fasta, records = [], [], []
        for key, tr in numbered(self._spool):
            for tag, allele in (("REF", tr.ref), ("ALT", tr.alt)):
                names.append(("%s|%s" % (key, tag), len(allele)))
                fasta.append(">%s|%s\n%s\n" % (key, tag, allele))
            for k, read in enumerate(tr.reads):
                line = sam_record(key, k, read)
                if line is not None:
                    records.append(line + "\n")
        with open(self.stem + ".fa", "w") as f:
            f.write("".join(fasta))
        with open(self.stem + ".sam", "w") as f:
            f.write("@HD\tVN:1.6\tSO:unknown\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % nl for nl in names) + "".join(records))
        self._spool = {}
        return self.stem + ".sam", self.stem + ".fa"


def votes(d_ref, d_alt) -> List[int]:
    """Per read its diff = d_ref - d_alt: the read votes ALT iff diff >= MARGIN, REF iff diff <= -MARGIN, else it makes no call."""
    return [int(r) - int(a) for r, a in zip(d_ref, d_alt)]


def counts(diffs):
    """(ALT, REF, NC) of a list of diffs."""
    alt = sum(1 for v in diffs if v >= MARGIN)
    ref = sum(1 for v in diffs if v <= -MARGIN)
    return alt, ref, len(diffs) - alt - ref


class Payload(list):
    """The reads' diffs, in read order.  What the run's other options know of the locus rides on it, None unless set: `traces`
    (a Traces, on the rank that scored it) and, one a section, `polish`, `junction` and `revote`."""
    traces = polish = junction = revote = None

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


class Section:
    """What one `--realign-*` option adds behind the seven columns (polish.SECTION, junction.SECTION, revote.SECTION): `attr`,
    the flag of Options that asks for it and the attribute of the Payload its object rides on; `INFO`, its own ##INFO tuples, and
    `COLUMNS`; `columns(p)`, its own fields of a payload or of None, gate included; `floats(obj)`, its object as floats for the
    gather, and `read(flat, at)` -> (obj, next), the object back from the floats that start at `at`."""

    def __init__(self, attr, info, columns, floats, read):
        self.attr, self.INFO, self.columns, self.floats, self.read = attr, tuple(info), columns, floats, read
        self.COLUMNS = tuple(i[0] for i in self.INFO)


class Chain:
    """The surface of a `--realign` run for modes.Mode and the VCF writer: the seven columns, then those of `sections`, in order.
    pack: `pack`'s floats, then per section 0 where the payload carries none of it, or 1 and the section's floats; unpack walks
    that list once, every section reading its own floats from where the one before it stopped."""

    def __init__(self, sections=()):
        self.SECTIONS = tuple(sections)
        self.INFO = INFO + tuple(i for s in self.SECTIONS for i in s.INFO)
        self.COLUMNS = tuple(i[0] for i in self.INFO)

    def columns(self, p) -> List[str]:
        return columns(p) + [c for s in self.SECTIONS for c in s.columns(p)]

    def pack(self, p) -> List[float]:
        flat = pack(p)
        for s in self.SECTIONS if p is not None else ():
            obj = getattr(p, s.attr)
            flat += [0.0] if obj is None else [1.0] + [float(v) for v in s.floats(obj)]
        return flat

    def unpack(self, flat) -> Optional[Payload]:
        p = unpack(flat)
        at = 1 + len(p) if p is not None else 0
        for s in self.SECTIONS if p is not None else ():
            at += 1
            if len(flat) >= at and int(flat[at - 1]) == 1:
                obj, at = s.read(flat, at)
                setattr(p, s.attr, obj)
        return p

    def columns_many(self, payloads) -> List[List[str]]:
        return [self.columns(p) for p in payloads]

"""Seeded synthetic genomes, SV loci and PacBio-like reads.

Everything here is the build's own generator: i.i.d. uniform ACGT contigs, SVs
implanted by string surgery, reads sampled from the ref or alt haplotype with
CLR-like errors (1 % sub / 8 % ins / 4 % del by default) and a CIGAR that is
exact up to the left edge of the SV (all the reference ever walks, see
vapor_vali/Simple_function.pyx:309-337).  The records are served to host code
through `vapor_amd.seqio.MemorySamtools`, which speaks the two samtools text
formats the reference parses (SF:339-354, SF:1203-1217).

No reference code is used or needed here.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = {i: None for i in range(256)}
_COMP.update({ord(a): b for a, b in zip("ACGTNacgtn", "TGCANtgcan")})


def random_dna(rng: np.random.Generator, n: int) -> str:
    return _ACGT[rng.integers(0, 4, size=n)].tobytes().decode("ascii")


def revcomp(seq: str) -> str:
    """Reverse complement over ACGTN/acgtn; other characters are dropped, as the
    reference's `complementary` does (SF:471-478)."""
    return seq.translate(_COMP)[::-1]


def _rle_cigar(ops: np.ndarray) -> str:
    # ops: uint8 array of b'M', b'I', b'D'
    if ops.size == 0:
        return "*"
    change = np.flatnonzero(ops[1:] != ops[:-1]) + 1
    starts = np.concatenate(([0], change))
    ends = np.concatenate((change, [ops.size]))
    # "<run length><op>" for every run, formatted by numpy rather than one str.__mod__ per run
    return "".join(np.char.add((ends - starts).astype("U"), ops[starts].view("S1").astype("U")).tolist())


def mutate(rng: np.random.Generator, seg: str, sub: float = 0.01, ins: float = 0.08,
           dele: float = 0.04, cigar: bool = True) -> Tuple[str, str]:
    """Apply CLR-like errors to `seg`; returns (read, cigar relative to seg; "" when `cigar` is off - the random
    stream is the same either way).

    The first base is always kept as a match so that POS is the first aligned base."""
    n = len(seg)
    if n == 0:
        return "", "*"
    b = np.frombuffer(seg.encode("ascii"), dtype=np.uint8)
    u = rng.random(n)
    is_del = u < dele
    is_sub = (u >= dele) & (u < dele + sub)
    is_ins = rng.random(n) < ins
    is_del[0] = False
    is_sub[0] = False
    # substituted bases: rotate within ACGT when the base is ACGT, else keep
    code = np.full(256, 255, dtype=np.uint8)
    code[_ACGT] = np.arange(4, dtype=np.uint8)
    c = code[b]
    rot = rng.integers(1, 4, size=n).astype(np.uint8)
    subbed = np.where((c < 4) & is_sub, _ACGT[(c + rot) & 3], b)
    ins_b = _ACGT[rng.integers(0, 4, size=n)]
    keep = ~is_del
    # output layout: for each position p: [base if kept][inserted base if is_ins]
    cnt = keep.astype(np.int64) + is_ins.astype(np.int64)
    off = np.concatenate(([0], np.cumsum(cnt)))
    out = np.empty(off[-1], dtype=np.uint8)
    out[off[:-1][keep]] = subbed[keep]
    ins_pos = off[:-1] + keep.astype(np.int64)
    out[ins_pos[is_ins]] = ins_b[is_ins]
    # cigar ops: per position M or D, then I
    if not cigar:
        return out.tobytes().decode("ascii"), ""
    opcnt = 1 + is_ins.astype(np.int64)
    ooff = np.concatenate(([0], np.cumsum(opcnt)))
    ops = np.empty(ooff[-1], dtype=np.uint8)
    ops[ooff[:-1]] = np.where(keep, ord("M"), ord("D"))
    ops[(ooff[:-1] + 1)[is_ins]] = ord("I")
    return out.tobytes().decode("ascii"), _rle_cigar(ops)


@dataclasses.dataclass
class SamRecord:
    qname: str
    rname: str
    pos: int          # 1-based leftmost aligned base
    cigar: str
    seq: str
    ref_span: int     # reference bases the alignment is taken to cover (for region overlap)
    tags: Optional[dict] = None      # optional fields, e.g. {"HP": 1, "PS": 7} (vapor_amd.phase: encode_aux, sam_fields)
    flag: int = 0                    # FLAG and MAPQ, what the read filter looks at
    mapq: int = 60

    def tag_fields(self) -> List[str]:
        """The optional fields as SAM text (`HP:i:1`, ...)."""
        if not self.tags:
            return []
        from .phase import sam_fields
        return sam_fields(self.tags)

    def line(self) -> str:
        return "\t".join([self.qname, str(self.flag), self.rname, str(self.pos), str(self.mapq), self.cigar,
                          "*", "0", "0", self.seq or "*", "*"] + self.tag_fields())


@dataclasses.dataclass
class Locus:
    """One SV call in a private contig (0-based half-open internals, 1-based text outside)."""
    chrom: str
    svtype: str                   # DEL | TANDUP | INV | INS | DISDUP | DUP_INV | DEL_INV
    start: int                    # as written to BED/VCF column 2
    end: int                      # column 3
    svid: str
    ins_seq: Optional[str] = None
    extra: Optional[dict] = None  # insert_point etc. for the complex types


class SynthWorld:
    """Contigs + aligned reads, addressable the way samtools addresses them."""

    def __init__(self) -> None:
        self.contigs: Dict[str, str] = {}
        self.reads: Dict[str, List[SamRecord]] = {}
        self.loci: List[Locus] = []

    # -- samtools-like accessors -------------------------------------------------
    def fetch(self, chrom: str, start: int, end: int) -> str:
        """1-based inclusive, clipped to the contig like `samtools faidx`."""
        s = self.contigs[chrom]
        start = max(int(start), 1)
        end = min(int(end), len(s))
        if end < start:
            return ""
        return s[start - 1:end]

    def overlapping(self, chrom: str, start: int, end: int) -> List[SamRecord]:
        out = []
        for r in self.reads.get(chrom, ()):
            if r.pos <= end and r.pos + r.ref_span - 1 >= start:
                out.append(r)
        return out


def apply_sv(ref: str, svtype: str, s: int, e: int, ins_seq: Optional[str] = None,
             ins_point: Optional[int] = None) -> str:
    """Alt haplotype of a whole contig. `s`,`e` are the BED columns; the SV block is
    contig[s:e] in 0-based half-open terms (the reference treats faidx s..e loosely;
    the generator only has to be self-consistent)."""
    blk = ref[s:e]
    if svtype == "DEL":
        return ref[:s] + ref[e:]
    if svtype in ("TANDUP", "DUP"):
        return ref[:e] + blk + ref[e:]
    if svtype == "INV":
        return ref[:s] + revcomp(blk) + ref[e:]
    if svtype == "INS":
        return ref[:s] + (ins_seq or "") + ref[s:]
    if svtype == "DISDUP":
        p = int(ins_point)
        return ref[:p] + blk + ref[p:]
    if svtype == "DUP_INV":
        p = int(ins_point)
        return ref[:p] + revcomp(blk) + ref[p:]
    if svtype == "DEL_INV":
        # delete [s, m) and invert [m, e), m carried in ins_point
        m = int(ins_point)
        return ref[:s] + revcomp(ref[m:e]) + ref[e:]
    raise ValueError(svtype)


_SPAN_TABLES = None


def simulate_span_tables() -> dict:
    """The SV span distribution of the reference's simulated truth sets (simulate/Structural_Variants_het: spans 50 bp - 100 kb,
    median ~2.8 kb, 7-10 % of the deletions and inversions >= 10 kb; tandem duplications below 5 kb; insertion lengths from the
    element names) as quantile tables - vapor_amd/data/simulate_spans.json, written by oracle/gen_span_dist.py in the build
    container (data only)."""
    global _SPAN_TABLES
    if _SPAN_TABLES is None:
        import json
        import os
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "simulate_spans.json")) as f:
            _SPAN_TABLES = json.load(f)
    return _SPAN_TABLES


def draw_span(rng, table: dict) -> int:
    """One value from a quantile table: inverse CDF, linear between quantiles."""
    q = table["quantiles"]
    x = float(rng.random()) * (len(q) - 1)
    lo = min(int(x), len(q) - 2)
    return int(round(q[lo] + (q[lo + 1] - q[lo]) * (x - lo)))


def make_world(seed: int, n_loci: int, svtypes: Sequence[str] = ("DEL", "TANDUP"),
               span_range: Tuple[int, int] = (200, 3000), read_len: int = 6000,
               n_reads: int = 12, alt_fraction: float = 0.5, lead: int = 300,
               contig_pad: int = 2000, errors: Tuple[float, float, float] = (0.01, 0.08, 0.04),
               chrom_prefix: str = "c", ins_len_range: Tuple[int, int] = (100, 600), span_dist: str = None,
               span_max: int = 100000, spans: Sequence[int] = None) -> SynthWorld:
    """Build `n_loci` independent loci, one contig each.

    Reads start 1..`lead` bases left of the scored window's left edge (SV start minus the
    500 bp flank) so that the reference's POS<=start filter keeps them, and are
    `read_len` haplotype bases long before errors.
    span_dist = "simulate": spans (and insertion lengths) are drawn from the distribution of the reference's simulated truth
    sets per SV type (simulate_span_tables) instead of uniformly from `span_range`; a span above `span_max` is drawn again."""
    rng = np.random.default_rng(seed)
    w = SynthWorld()
    tables = simulate_span_tables() if span_dist == "simulate" else None
    if span_dist not in (None, "simulate"):
        raise ValueError("span_dist: None or 'simulate'")
    for li in range(n_loci):
        svtype = svtypes[li % len(svtypes)]
        if spans is not None:
            span = int(spans[li % len(spans)])             # (given locus by locus)
        elif tables is not None:
            tb = tables["simple"].get(svtype) or tables["simple"]["DEL"]
            span = draw_span(rng, tb)
            while span > span_max or span < 1:
                span = draw_span(rng, tb)
        else:
            span = int(rng.integers(span_range[0], span_range[1] + 1))
        flank = min(500, span)
        left = flank + lead + 50
        # (a span the drivers score by its junction windows only - 10 kb and more, SF:1706 - needs no room for the alt
        # haplotype's doubled block behind it)
        clen = left + (3 if (span < 10000 or svtype not in ("DEL", "INV")) else 1) * span + read_len + contig_pad
        chrom = "%s%d" % (chrom_prefix, li + 1)
        ref = random_dna(rng, clen)
        s = left
        e = s + span
        ins_seq = None
        ins_point = None
        extra = None
        if svtype == "INS":
            ilen = draw_span(rng, tables["insertion_length"]) if tables is not None else int(rng.integers(ins_len_range[0], ins_len_range[1] + 1))
            ilen = max(ilen, 1)
            ins_seq = random_dna(rng, ilen)
            e = s + 1
            flank = min(500, ilen)
        elif svtype in ("DISDUP", "DUP_INV"):
            ins_point = e + int(rng.integers(50, max(51, span)))
            extra = {"insert_point": ins_point}
        elif svtype == "DEL_INV":
            ins_point = s + span // 2
            extra = {"mid": ins_point}
        alt = apply_sv(ref, svtype, s, e, ins_seq, ins_point)
        w.contigs[chrom] = ref
        recs: List[SamRecord] = []
        win_left = s - flank  # 1-based coordinate the reference uses as window start
        for ri in range(n_reads):
            from_alt = rng.random() < alt_fraction
            hap = alt if from_alt else ref
            a = win_left - 1 - int(rng.integers(1, lead + 1))
            a = max(a, 0)
            b = min(a + read_len, len(hap))
            read, cigar = mutate(rng, hap[a:b], *errors)
            recs.append(SamRecord("r%d_%d%s" % (li + 1, ri, "a" if from_alt else "r"), chrom,
                                  a + 1, cigar, read, b - a))
        w.reads[chrom] = recs
        w.loci.append(Locus(chrom, svtype, s, e, "sv%d" % (li + 1), ins_seq, extra))
    return w


def bed_text(world: SynthWorld) -> str:
    """5+ column BED as `bed_info_readin` expects it today (vapor_vali/vapor:22-50)."""
    rows = []
    for l in world.loci:
        t = {"TANDUP": "DUP"}.get(l.svtype, l.svtype)
        if l.svtype == "INS":
            rows.append("\t".join([l.chrom, str(l.start), str(l.end), l.svid, "INS", l.ins_seq]))
        elif l.svtype in ("DEL", "TANDUP", "INV"):
            rows.append("\t".join([l.chrom, str(l.start), str(l.end), l.svid, t]))
    return "\n".join(rows) + "\n"


def vcf_text(world: SynthWorld, header: bool = True) -> str:
    """Minimal VCF with the INFO keys `vcf_list_readin` reads (vapor_vali/vapor:127-202,
    README.md:79-82 for the complex types)."""
    out = ["##fileformat=VCFv4.1", "##INFO=<ID=SVTYPE,Number=1,Type=String,Description=\"Type of SV\">",
           "##INFO=<ID=END,Number=1,Type=Integer,Description=\"End\">", "##source=vapor_amd.synth",
           "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE"] if header else []
    for l in world.loci:
        info = "SVTYPE=%s;END=%d" % ({"TANDUP": "DUP"}.get(l.svtype, l.svtype), l.end)
        alt = "<%s>" % l.svtype
        if l.svtype == "INS":
            info = "SVTYPE=INS;END=%d;SVLEN=%d;SEQ=%s" % (l.end, len(l.ins_seq), l.ins_seq)
            alt = "<INS>"
        elif l.svtype in ("DISDUP", "DUP_INV"):
            info += ";insert_point=%s:%d" % (l.chrom, l.extra["insert_point"])
        elif l.svtype == "DEL_INV":
            m = l.extra["mid"]
            info += ";del=%s:%d-%d;inv=%s:%d-%d" % (l.chrom, l.start, m, l.chrom, m, l.end)
        out.append("\t".join([l.chrom, str(l.start), l.svid, "N", alt, ".", "PASS", info,
                              "GT", "0/1"]))
    return "\n".join(out) + "\n"


# ---------------------------------------------------------------------------
# kernel-level synthetic shapes (bench / parity at BASELINE sizes)
# ---------------------------------------------------------------------------

def make_pairs(seed: int, n_alleles: int, reads_per_allele: int, read_len: int, allele_len: int,
               errors: Tuple[float, float, float] = (0.01, 0.08, 0.04),
               sv: bool = True) -> Tuple[List[str], List[str], List[Tuple[int, int]]]:
    """`n_alleles` windows of `allele_len` bases, each with `reads_per_allele` noisy reads of
    ~`read_len` bases drawn from inside the window (half of the alleles carry a deletion
    relative to the haplotype the reads come from when `sv`), returning
    (alleles, reads, [(read_idx, allele_idx)...])."""
    rng = np.random.default_rng(seed)
    alleles: List[str] = []
    reads: List[str] = []
    pairs: List[Tuple[int, int]] = []
    for ai in range(n_alleles):
        a = random_dna(rng, allele_len)
        alleles.append(a)
        hap = a
        if sv and (ai & 1):
            cut = int(rng.integers(allele_len // 4, allele_len // 2))
            ln = int(rng.integers(50, 2000))
            hap = a[:cut] + a[cut + ln:]
        for _ in range(reads_per_allele):
            st = int(rng.integers(0, max(1, len(hap) - read_len)))
            r, _c = mutate(rng, hap[st:st + read_len], *errors)
            reads.append(r[:read_len])
            pairs.append((len(reads) - 1, ai))
    return alleles, reads, pairs


def world_from_json(d: dict) -> SynthWorld:
    """Inverse of the fixture layout written by oracle/gen_golden.py (world_to_json)."""
    w = SynthWorld()
    w.contigs = dict(d["contigs"])
    w.reads = {c: [SamRecord(q, c, pos, cig, seq, span) for q, pos, cig, seq, span in rs]
               for c, rs in d["reads"].items()}
    w.loci = [Locus(*l) for l in d["loci"]]
    return w


class VirtualContig:
    """A chromosome-sized i.i.d. ACGT sequence that is never materialised: 4 kb blocks are generated
    on demand from (seed, block index).  Supports len() and slicing like a str."""
    BLOCK = 4096

    def __init__(self, seed: int, length: int):
        self.seed, self.length = int(seed), int(length)
        self._cache: Dict[int, str] = {}

    def __len__(self) -> int:
        return self.length

    def _block(self, b: int) -> str:
        s = self._cache.get(b)
        if s is None:
            s = random_dna(np.random.default_rng([self.seed, b]), self.BLOCK)
            if len(self._cache) > 4096:
                self._cache.clear()
            self._cache[b] = s
        return s

    def __getitem__(self, sl) -> str:
        if not isinstance(sl, slice):
            raise TypeError("VirtualContig supports slices only")
        a, b, _ = sl.indices(self.length)
        if b <= a:
            return ""
        parts = [self._block(k) for k in range(a // self.BLOCK, (b - 1) // self.BLOCK + 1)]
        s = "".join(parts)
        off = a - (a // self.BLOCK) * self.BLOCK
        return s[off:off + (b - a)]


def make_world_from_bed(rows: Sequence[Sequence], seed: int, contig_len: int = 135534747, n_reads: int = 10,
                        alt_fraction: float = 0.5, lead: int = 250,
                        errors: Tuple[float, float, float] = (0.01, 0.08, 0.04)) -> SynthWorld:
    """Loci at given genome coordinates (rows of chrom, start, end, TYPE) on virtual contigs, with reads
    sampled around every locus - BASELINE.json configs[0]: the reference's vapor_test.bed needs a BAM
    and hg19 that are not bundled, so the plumbing runs on a stand-in genome."""
    rng = np.random.default_rng(seed)
    w = SynthWorld()
    for li, row in enumerate(rows):
        chrom, s, e, svtype = row[0], int(row[1]), int(row[2]), {"DUP": "TANDUP"}.get(row[3], row[3])
        if chrom not in w.contigs:
            w.contigs[chrom] = VirtualContig(seed * 1000003 + len(w.contigs), contig_len)
            w.reads[chrom] = []
        span = e - s
        flank = min(500, span)
        r0 = s - flank - lead - 50                       # 0-based start of the local window
        read_len = 2 * flank + 2 * span + lead + 400
        local = w.contigs[chrom][r0:r0 + read_len + 3 * span + 2000]
        ls, le = s - r0, e - r0
        alt = apply_sv(local, svtype, ls, le)
        for ri in range(n_reads):
            from_alt = rng.random() < alt_fraction
            hap = alt if from_alt else local
            a = (s - flank) - r0 - 1 - int(rng.integers(1, lead + 1))
            b = min(a + read_len, len(hap))
            read, cigar = mutate(rng, hap[a:b], *errors)
            w.reads[chrom].append(SamRecord("v%d_%d%s" % (li + 1, ri, "a" if from_alt else "r"), chrom,
                                            r0 + a + 1, cigar, read, b - a))
        w.loci.append(Locus(chrom, svtype, s, e, "sv%d" % (li + 1)))
    return w


# ---------------------------------------------------------------------------
# complex SV types of the VCF path (BASELINE.json configs[3]): DISDUP, DUP_INV, DEL_INV, Other=
# ---------------------------------------------------------------------------

def _add_reads(rng, w: SynthWorld, chrom: str, hap_ref: str, hap_alt: str, anchor: int, read_len: int, n_reads: int,
               alt_fraction: float, lead: int, errors, tag: str) -> None:
    """`n_reads` reads that start 1..`lead` bases left of the 1-based window start `anchor`."""
    recs = w.reads.setdefault(chrom, [])
    for ri in range(n_reads):
        from_alt = rng.random() < alt_fraction
        hap = hap_alt if from_alt else hap_ref
        a = max(anchor - 1 - int(rng.integers(1, lead + 1)), 0)
        b = min(a + read_len, len(hap))
        read, cigar = mutate(rng, hap[a:b], *errors)
        recs.append(SamRecord("%s_%d%s" % (tag, ri, "a" if from_alt else "r"), chrom, a + 1, cigar, read, b - a))


def make_complex_world(seed: int, specs: Sequence[dict], n_reads: int = 8, alt_fraction: float = 0.5, lead: int = 250,
                       errors: Tuple[float, float, float] = (0.01, 0.08, 0.04), chrom_prefix: str = "x") -> SynthWorld:
    """One private contig (two for an inter-contig duplication) per spec.  Spec keys:
      type   DUP_INV | DISDUP | DEL_INV | OTHER
      a      length of the duplicated / first block
      gap    DUP_INV / DISDUP: distance from the block's end to the insert point (negative: the insert point lies
             that far left of the block's start); `inside`: insert point this far inside the block
      b      DEL_INV: length of the second block; OTHER: length of block b
      order  DEL_INV: "del,inv" or "inv,del"; `apart`: bases between the two blocks (the reference wants < 100)
      other  OTHER: (ref structure, alt structure), e.g. ("ab/ab", "b/b^")
      xchrom DISDUP / DUP_INV: insert point on a contig of its own, at this coordinate
      n_reads / alt_fraction override the defaults.
    Duplicated blocks are kept short against the distance to their copy so that the self dot plot of the alt
    window stays below the 10 % lower-triangle share at which the reference starts its unseeded X-means
    (qual_check_repetitive_region, SF:1165)."""
    rng = np.random.default_rng(seed)
    w = SynthWorld()
    for li, sp in enumerate(specs):
        t = sp["type"]
        chrom = "%s%d" % (chrom_prefix, li + 1)
        a = int(sp["a"])
        nr = int(sp.get("n_reads", n_reads))
        af = float(sp.get("alt_fraction", alt_fraction))
        left = 500 + lead + 80
        tag = "q%d" % (li + 1)
        if t in ("DUP_INV", "DISDUP"):
            s, e = left, left + a
            flank = min(500, a)
            rcb = t == "DUP_INV"
            if "xchrom" in sp:
                # the copy lands on another contig
                p = int(sp["xchrom"])
                ref = random_dna(rng, e + 3000)
                xc = chrom + "i"
                xref = random_dna(rng, p + a + 4000)
                blk = ref[s:e]
                xalt = xref[:p] + (revcomp(blk) if rcb else blk) + xref[p:]
                w.contigs[chrom] = ref
                w.contigs[xc] = xref
                w.reads.setdefault(chrom, [])
                _add_reads(rng, w, xc, xref, xalt, p - flank, 2 * flank + a + lead + 600, nr, af, lead, errors, tag)
                w.loci.append(Locus(chrom, t, s, e, "cx%d" % (li + 1), None, {"insert_point": p, "insert_chrom": xc}))
                continue
            gap = int(sp.get("gap", 1200))
            if sp.get("inside"):
                p = s + int(sp["inside"])
            elif gap >= 0:
                p = e + gap
            else:
                left = left - gap
                s, e = left, left + a
                p = s + gap
            hi = max(e, p)
            ref = random_dna(rng, hi + 2 * a + 3000 + lead)
            blk = ref[s:e]
            alt = ref[:p] + (revcomp(blk) if rcb else blk) + ref[p:]
            w.contigs[chrom] = ref
            far = hi - min(s, p) >= 10000
            if far:
                anchor, rl = p - flank, 2 * flank + a + lead + 600
            else:
                anchor, rl = min(s, p) - flank, (hi - min(s, p)) + a + 2 * flank + lead + 500
            _add_reads(rng, w, chrom, ref, alt, anchor, rl, nr, af, lead, errors, tag)
            w.loci.append(Locus(chrom, t, s, e, "cx%d" % (li + 1), None, {"insert_point": p, "insert_chrom": chrom}))
        elif t == "DEL_INV":
            b = int(sp["b"])
            apart = int(sp.get("apart", 0))
            s = left
            m1 = s + a                    # end of the first block
            m0 = m1 + apart               # start of the second
            e = m0 + b
            ref = random_dna(rng, e + a + b + 3000 + lead)
            first, second = sp.get("order", "del,inv").split(",")
            blocks = [(s, m1, first), (m0, e, second)]
            def piece(x0, x1, kind):
                return revcomp(ref[x0:x1]) if kind == "inv" else ""

            alt = ref[:s] + piece(*blocks[0]) + ref[m1:m0] + piece(*blocks[1])
            alt += ref[e:]
            w.contigs[chrom] = ref
            flank = min(500, e - s)
            if e - s >= 10000:
                anchor, rl = s - flank, 2 * flank + lead + 700
            else:
                anchor, rl = s - flank, (e - s) + 2 * flank + lead + 500
            _add_reads(rng, w, chrom, ref, alt, anchor, rl, nr, af, lead, errors, tag)
            w.loci.append(Locus(chrom, t, s, e, "cx%d" % (li + 1), None,
                                {"blocks": [[x0, x1, kind] for (x0, x1, kind) in blocks]}))
        elif t == "OTHER":
            b = int(sp["b"])
            s = left
            m = s + a
            e = m + b
            ref = random_dna(rng, e + a + b + 3000 + lead)
            ref_s, alt_s = sp["other"]
            blk = {"a": ref[s:m], "b": ref[m:e]}
            alleles = [x for x in alt_s.split("/") if x not in ref_s.split("/")] or [ref_s.split("/")[0]]
            haps = []
            for al in alleles:
                mid, prev = "", None
                for ch in al:
                    if ch == "^":
                        mid = mid[:len(mid) - len(blk[prev])] + revcomp(blk[prev])
                    else:
                        mid += blk[ch]
                        prev = ch
                haps.append(ref[:s] + mid + ref[e:])
            w.contigs[chrom] = ref
            flank = min(500, e - s)
            rl = 2 * (e - s) + 2 * flank + lead + 500
            recs = w.reads.setdefault(chrom, [])
            for ri in range(nr):
                from_alt = rng.random() < af
                hap = haps[ri % len(haps)] if from_alt else ref
                a0 = max(s - flank - 1 - int(rng.integers(1, lead + 1)), 0)
                b0 = min(a0 + rl, len(hap))
                read, cigar = mutate(rng, hap[a0:b0], *errors)
                recs.append(SamRecord("%s_%d%s" % (tag, ri, "a" if from_alt else "r"), chrom, a0 + 1, cigar, read, b0 - a0))
            w.loci.append(Locus(chrom, t, s, e, "cx%d" % (li + 1), None, {"other": [ref_s, alt_s], "bps": [s, m, e]}))
        else:
            raise ValueError(t)
    return w


BND_FORMS = ("3to5", "3to3", "5to3", "5to5")


def bnd_alt(form: str, ref_base: str, ins: str, chrom: str, pos: int) -> str:
    """The VCF 4.x ALT of a breakend whose partner is chrom:pos: t[p[ 3to5, t]p] 3to3, ]p]t 5to3, [p[t 5to5."""
    p = "%s:%d" % (chrom, pos)
    return {"3to5": ref_base + ins + "[" + p + "[", "3to3": ref_base + ins + "]" + p + "]",
            "5to3": "]" + p + "]" + ins + ref_base, "5to5": "[" + p + "[" + ins + ref_base}[form]


def _clipped_reads(rng, w, chrom, side, at, flank_seq, n, read_len, lead, errors, tag, ref_fraction=0.0):
    """n reads on `chrom` that carry a junction: side 'R' = aligned up to `at` (1-based) and soft-clipped after it (xM yS, the
    clip = the start of `flank_seq`); side 'L' = soft-clipped before `at` and aligned from it on (yS xM, the clip = the end of
    `flank_seq`).  A read drawn as a reference read (`ref_fraction`) is the contig itself across `at`, unclipped."""
    c = w.contigs[chrom]
    recs = w.reads.setdefault(chrom, [])
    for ri in range(n):
        from_ref = rng.random() < ref_fraction
        if side == "R":
            a0 = max(at - 500 - 1 - int(rng.integers(1, lead + 1)), 0)     # from before the window's start (SF:345)
            if from_ref:
                b0 = min(a0 + read_len, len(c))
                read, cig = mutate(rng, c[a0:b0], *errors)
                recs.append(SamRecord("%s_R%dr" % (tag, ri), chrom, a0 + 1, cig, read, b0 - a0))
                continue
            ra, ca = mutate(rng, c[a0:at], *errors)
            rt, _ = mutate(rng, flank_seq[:max(read_len - (at - a0), 0)], *errors, cigar=False)
            recs.append(SamRecord("%s_R%da" % (tag, ri), chrom, a0 + 1, ca + ("%dS" % len(rt) if rt else ""), ra + rt, at - a0))
        else:
            h = min(len(flank_seq), int(rng.integers(300, 500 + lead)))
            b0 = min(at - 1 + read_len - h, len(c))
            if from_ref:
                a0 = max(at - 1 - h, 0)
                read, cig = mutate(rng, c[a0:b0], *errors)
                recs.append(SamRecord("%s_L%dr" % (tag, ri), chrom, a0 + 1, cig, read, b0 - a0))
                continue
            rh, _ = mutate(rng, flank_seq[len(flank_seq) - h:], *errors, cigar=False)
            ra, ca = mutate(rng, c[at - 1:b0], *errors)
            recs.append(SamRecord("%s_L%da" % (tag, ri), chrom, at, ("%dS" % len(rh) if rh else "") + ca, rh + ra, b0 - at + 1))


def make_bnd_world(seed: int, forms: Sequence[str] = BND_FORMS, n_reads: int = 8, read_len: int = 2400, lead: int = 250,
                   ref_fraction: float = 0.0, ins: Sequence[str] = ("",), errors: Tuple[float, float, float] = (0.01, 0.08, 0.04),
                   chrom_prefix: str = "t") -> SynthWorld:
    """Translocation worlds: per junction two contigs of their own, A (<prefix><i>a) and B (<prefix><i>b), joined by a breakend
    of the given form - the record at A:p, its mate at B:q (VCF 4.x, bnd_alt), inserted bases ins[i % len(ins)] between the
    pieces, as the record at A:p writes them:

        3to5  t[B:q[   A up to p, then B from q on          5to3  ]B:q]t   B up to q, then A from p on
        3to3  t]B:q]   A up to p, then rc(B up to q)        5to5  [B:q[t   rc(B from q on), then A from p on

    A read on the piece that ends at the junction is aligned up to it and soft-clipped after it (xM yS); a read on the piece that
    starts there is soft-clipped before it (yS xM); SEQ holds the clipped bases.  Every side gets n_reads reads, a share
    `ref_fraction` of those on the right-clipped side drawn from the contig instead.  Loci: svtype 'BND', start = p,
    end = q, extra = {form, mate_chrom}.  (A generator of its own: make_world's draws stay as they are.)"""
    rng = np.random.default_rng(seed)
    w = SynthWorld()
    for li, form in enumerate(forms):
        if form not in BND_FORMS:
            raise ValueError(form)
        ca, cb = "%s%da" % (chrom_prefix, li + 1), "%s%db" % (chrom_prefix, li + 1)
        p = 1500 + int(rng.integers(0, 200))
        q = 1500 + int(rng.integers(0, 200))
        A = w.contigs[ca] = random_dna(rng, p + read_len + 400)
        B = w.contigs[cb] = random_dna(rng, q + read_len + 400)
        I = ins[li % len(ins)]
        tag = "j%d" % (li + 1)
        n_ref = ref_fraction
        if form == "3to5":          # A[:p] + I + B[q-1:]
            _clipped_reads(rng, w, ca, "R", p, I + B[q - 1:], n_reads, read_len, lead, errors, tag + "a", n_ref)
            _clipped_reads(rng, w, cb, "L", q, A[:p] + I, n_reads, read_len, lead, errors, tag + "b")
        elif form == "3to3":        # A[:p] + I + rc(B[:q]); from B: B[:q] + rc(I) + rc(A[:p])
            _clipped_reads(rng, w, ca, "R", p, I + revcomp(B[:q]), n_reads, read_len, lead, errors, tag + "a", n_ref)
            _clipped_reads(rng, w, cb, "R", q, revcomp(I) + revcomp(A[:p]), n_reads, read_len, lead, errors, tag + "b", n_ref)
        elif form == "5to3":        # B[:q] + I + A[p-1:]
            _clipped_reads(rng, w, cb, "R", q, I + A[p - 1:], n_reads, read_len, lead, errors, tag + "b", n_ref)
            _clipped_reads(rng, w, ca, "L", p, B[:q] + I, n_reads, read_len, lead, errors, tag + "a")
        else:                       # rc(B[q-1:]) + I + A[p-1:]; from B: rc(A[p-1:]) + rc(I) + B[q-1:]
            _clipped_reads(rng, w, ca, "L", p, revcomp(B[q - 1:]) + I, n_reads, read_len, lead, errors, tag + "a")
            _clipped_reads(rng, w, cb, "L", q, revcomp(A[p - 1:]) + revcomp(I), n_reads, read_len, lead, errors, tag + "b")
        for c in (ca, cb):
            w.reads.setdefault(c, []).sort(key=lambda r: r.pos)
        w.loci.append(Locus(ca, "BND", p, q, "bnd%d" % (li + 1), I, {"form": form, "mate_chrom": cb}))
    return w


def make_junction_world(seed: int, svtypes: Sequence[str] = ("DEL", "INV", "TANDUP"), span: int = 12000, n_reads: int = 12,
                        read_len: int = 2400, lead: int = 250, ref_fraction: float = 0.25,
                        errors: Tuple[float, float, float] = (0.01, 0.08, 0.04), chrom_prefix: str = "k") -> SynthWorld:
    """Long DEL / INV / TANDUP loci (a contig each, BED columns s and e = s + span) whose junctions are read from BOTH sides, the
    way an aligner reports a long read across a junction: the piece that ends there aligned and soft-clipped after it (xM yS),
    the piece that starts there soft-clipped before it (yS xM) - make_world's reads all start left of the first breakpoint.
    Per junction side n_reads reads, a share ref_fraction of them the contig itself.  DEL: A = ref[:s] + ref[e:], one junction;
    TANDUP: ref[:e] + ref[s:], one junction; INV: ref[:s] + rc(ref[s:e]) + ref[e:], two junctions, each also seen from the
    inverted strand."""
    rng = np.random.default_rng(seed)
    w = SynthWorld()
    for li in range(len(svtypes)):
        t = svtypes[li]
        c = "%s%d" % (chrom_prefix, li + 1)
        s = 1500 + int(rng.integers(0, 200))
        e = s + int(span)
        ref = w.contigs[c] = random_dna(rng, e + read_len + 600)
        tag = "g%d" % (li + 1)
        if t == "DEL":
            sides = [("R", s, ref[e:]), ("L", e + 1, ref[:s])]
        elif t in ("TANDUP", "DUP"):
            t = "TANDUP"
            sides = [("R", e, ref[s:]), ("L", s + 1, ref[:e])]
        elif t == "INV":
            blk = revcomp(ref[s:e])
            sides = [("R", s, blk), ("R", e, revcomp(ref[:s])), ("L", e + 1, blk), ("L", s + 1, revcomp(ref[e:]))]
        else:
            raise ValueError(t)
        for k, (side, at, other) in enumerate(sides):
            _clipped_reads(rng, w, c, side, at, other, n_reads, read_len, lead, errors, "%s%s" % (tag, "abcd"[k]), ref_fraction)
        w.reads[c].sort(key=lambda r: r.pos)
        w.loci.append(Locus(c, t, s, e, "jn%d" % (li + 1)))
    return w


DEPTH_SPECS = (("DEL", 600, "hom"), ("DEL", 1500, "het"), ("TANDUP", 900, "het"), ("TANDUP", 1200, "hom"), ("INV", 700, "het"),
               ("DEL", 24000, "het"), ("TANDUP", 22000, "het"))


def _noisy(rng, seg: str, errors) -> Tuple[str, str]:
    """`seg` read with substitutions, insertions and deletions at the rates `errors` = (sub, ins, del): (read, CIGAR with M, X, I
    and D).  The first and the last base are matches, so that the piece starts and ends on an aligned base."""
    sub, ins, dele = errors
    n = len(seg)
    b = np.frombuffer(seg.encode("ascii"), dtype=np.uint8)
    u = rng.random(n)
    kind = np.where(u < dele, ord("D"), np.where(u < dele + sub, ord("X"), ord("M"))).astype(np.uint8)
    is_ins = rng.random(n) < ins
    kind[0] = kind[-1] = ord("M")
    is_ins[-1] = False
    code = np.full(256, 0, dtype=np.uint8)
    code[_ACGT] = np.arange(4, dtype=np.uint8)
    base = np.where(kind == ord("X"), _ACGT[(code[b] + rng.integers(1, 4, size=n).astype(np.uint8)) & 3], b)
    ins_b = _ACGT[rng.integers(0, 4, size=n)]
    keep = kind != ord("D")
    cnt = keep.astype(np.int64) + is_ins.astype(np.int64)
    off = np.concatenate(([0], np.cumsum(cnt)))
    out = np.empty(off[-1], dtype=np.uint8)
    out[off[:-1][keep]] = base[keep]
    out[(off[:-1] + keep.astype(np.int64))[is_ins]] = ins_b[is_ins]
    ooff = np.concatenate(([0], np.cumsum(1 + is_ins.astype(np.int64))))
    ops = np.empty(ooff[-1], dtype=np.uint8)
    ops[ooff[:-1]] = kind
    ops[(ooff[:-1] + 1)[is_ins]] = ord("I")
    return out.tobytes().decode("ascii"), _rle_cigar(ops)


def make_depth_world(seed: int, specs: Sequence[Tuple[str, int, str]] = DEPTH_SPECS, layers: int = 4, read_len: int = 1000,
                     margin: int = 3000, errors: Optional[Tuple[float, float, float]] = None, short_del: int = 2000,
                     chrom_prefix: str = "d") -> SynthWorld:
    """A world whose read DEPTH means something (`--depth`; the other worlds only hold reads that start just
    left of a window).  Per spec (svtype, span L, 'hom' | 'het') a contig of margin + L + margin bases with the event on bases
    [margin + 1, margin + L] (the BED columns), and two haplotypes, each TILED with reads: `layers` layers a haplotype, layer k
    cut every read_len bases from offset k * read_len // layers, so that every base of a haplotype is in exactly `layers`
    reads and a diploid contig has depth 2 * layers.  A 'het' locus has one reference and one alt haplotype, a 'hom' one two
    alt haplotypes; an INV locus is read from two reference haplotypes.  The alt haplotype's reads are aligned as a mapper
    reports them: a read across a deletion of at most short_del bases carries it as a D; across a longer deletion, or across
    the junction of a tandem duplication (the end of the first copy, where the second starts), its longest piece is the primary
    record with the rest soft-clipped and every other piece a supplementary record (0x800) soft-clipped likewise; the second
    copy of a duplicated block aligns where the first does, which doubles the block's coverage.  Without errors every piece is
    one M and the depth of every base is known in closed form: outside the event 2 * layers; inside a DEL layers ('het') or 0
    ('hom'); inside a TANDUP 3 * layers ('het') or 4 * layers ('hom').  errors = (sub, ins, del): read errors as X, I and D."""
    rng = np.random.default_rng(seed)
    w = SynthWorld()
    for li, (t, span, zyg) in enumerate(specs):
        c = "%s%d" % (chrom_prefix, li + 1)
        s0, e0 = margin, margin + int(span)             # the event, 0-based half-open
        n = e0 + margin
        ref = w.contigs[c] = random_dna(rng, n)
        if t == "DEL":
            alt = [(0, s0), (e0, n)]
        elif t in ("TANDUP", "DUP"):
            t = "TANDUP"
            alt = [(0, e0), (s0, n)]
        elif t == "INV":
            alt = [(0, n)]
        else:
            raise ValueError(t)
        haps = [alt, alt] if zyg == "hom" else [[(0, n)], alt]
        recs = w.reads.setdefault(c, [])
        for h, segs in enumerate(haps):
            # the haplotype's segments in its own coordinates: (hap start, hap end, ref start)
            at, table = 0, []
            for lo, hi in segs:
                table.append((at, at + hi - lo, lo))
                at += hi - lo
            m = at
            for k in range(layers):
                cuts = sorted({0, m} | set(range((k * read_len) // layers, m, read_len)))
                for ri, (a, z) in enumerate(zip(cuts[:-1], cuts[1:])):
                    pieces = [(max(a, p0) - p0 + r0, min(z, p1) - p0 + r0) for p0, p1, r0 in table if min(z, p1) > max(a, p0)]
                    made = [(_noisy(rng, ref[lo:hi], errors) if errors else (ref[lo:hi], "%dM" % (hi - lo))) for lo, hi in pieces]
                    qname = "%s_h%d_l%d_r%d" % (c, h, k, ri)
                    seq = "".join(x[0] for x in made)
                    if len(pieces) == 2 and 0 < pieces[1][0] - pieces[0][1] <= short_del:
                        gap = pieces[1][0] - pieces[0][1]
                        recs.append(SamRecord(qname, c, pieces[0][0] + 1, made[0][1] + "%dD" % gap + made[1][1], seq, pieces[1][1] - pieces[0][0]))
                        continue
                    main = max(range(len(pieces)), key=lambda i: (pieces[i][1] - pieces[i][0], -i))
                    for i, (lo, hi) in enumerate(pieces):
                        left = sum(len(x[0]) for x in made[:i])
                        right = sum(len(x[0]) for x in made[i + 1:])
                        cg = ("%dS" % left if left else "") + made[i][1] + ("%dS" % right if right else "")
                        recs.append(SamRecord(qname, c, lo + 1, cg, seq, hi - lo, flag=0 if i == main else 0x800))
        recs.sort(key=lambda r: r.pos)
        w.loci.append(Locus(c, t, s0 + 1, e0, "dp%d" % (li + 1)))
    return w


SIGNATURE_SPECS = (("DEL", 600, "hom"), ("DEL", 1500, "het"), ("DEL", 6000, "het"), ("DEL", 12000, "hom"), ("TANDUP", 300, "het"),
                   ("TANDUP", 4000, "hom"), ("TANDUP", 15000, "het"), ("INV", 700, "het"), ("INV", 11000, "hom"), ("INS", 250, "het"),
                   ("INS", 3000, "hom"))


SUPPORT_SPECS = tuple((t, span, z) for t, span in (("DEL", 600), ("DEL", 12000), ("TANDUP", 300), ("TANDUP", 15000), ("INV", 700),
                                                   ("INV", 11000), ("INS", 250), ("INS", 3000)) for z in ("het", "hom", "ref"))


def make_signature_world(seed: int, specs: Sequence[Tuple[str, int, str]] = SIGNATURE_SPECS, layers: int = 4, read_len: int = 1000,
                         margin: int = 3000, short: int = 2000, guard: int = 100, jitter: Sequence[int] = (0,),
                         chrom_prefix: str = "s") -> SynthWorld:
    """A world whose split reads and CIGARs mean something (`--signatures`).  Per spec (svtype, span L, 'hom' |
    'het') a contig with the event on bases [margin + 1, margin + L] (an INS of L bases behind base `margin`, on a contig of
    2 * margin bases), and two haplotypes tiled with error-free reads as make_depth_world tiles them: `layers` layers a
    haplotype, 'het' one reference and one alt haplotype, 'hom' two alt haplotypes.  A cut that falls less than `guard` bases
    from a junction of the alt haplotype - for an event of at most `short` bases: anywhere from `guard` before the event to
    `guard` behind it - is left out, so that exactly one read of every layer crosses each junction, with `guard` bases at least
    on either side.  That read is aligned as a mapper reports it:
      DEL, L <= short: one record with an L D at cursor margin; longer: the piece left of the junction with the rest soft-clipped
        and the piece right of it likewise, the longer the primary and the other a supplementary record (0x800);
      TANDUP, L <= short: one record with an L I at cursor margin (left-aligned); longer: the piece that ends at margin + L and
        the piece that starts at margin, clipped primary and supplementary;
      INS, L <= short: one record with an L I at cursor margin; longer: the flanking pieces with the inserted bases soft-clipped
        (a read inside the insertion is not aligned and not in the file);
      INV: at each junction a forward piece and a reverse-strand piece (0x10), each with the rest soft-clipped.
    jitter: the alt reads of layer k report their breakpoints jitter[k % len(jitter)] bases to the right (a negative number: to
    the left), as alignments in a repeat do - so that the histograms have more than one bin.  With A = 1 ('het') or 2 ('hom')
    alt haplotypes every locus has A * layers reads at each junction, and its six columns are known in closed form:
      D / I carriers: L = R = 0, CG = A * layers;  split DEL, TANDUP, INS: L = R = A * layers, CG = 0;  INV: L = R = 2 * A * layers."""
    return _tiled_world(seed, specs, layers, read_len, margin, short, guard, jitter, chrom_prefix, False)


def make_support_world(seed: int, specs: Sequence[Tuple[str, int, str]] = SUPPORT_SPECS, layers: int = 4, read_len: int = 1000,
                       margin: int = 3000, short: int = 2000, guard: int = 100, jitter: Sequence[int] = (0,),
                       chrom_prefix: str = "u") -> SynthWorld:
    """A world whose reference alignments mean something as well (`--support`): make_signature_world's tiling
    with two changes.  The guard holds for every haplotype at the event's two reference breakpoints too: a cut nearer than
    `guard` (51 at least: support.F) to base `margin` or `margin + L` of the reference, wherever a haplotype carries that base
    with its neighbours, is left out - so every layer of such a haplotype has exactly one record that runs through the
    breakpoint, with `guard` bases on either side.  And there is a third zygosity, 'ref': two reference haplotypes.  With A = 0
    ('ref'), 1 ('het') or 2 ('hom') alt haplotypes the nine columns are known in closed form:
      ALT = A * layers - for an INV twice that: either junction has a forward and a reverse-strand record of every alt read;
      REFL = REFR = (2 - A) * layers for DEL, INS and INV, and for a TANDUP of at most `short` bases (its one record carries
        the I); 2 * layers for a longer TANDUP - the duplicated allele runs through both outer breakpoints contiguously;
      COVL = COVR = REF + the alt records that cover the breakpoint's base;  GT = 0/0, 0/1, 1/1 for A = 0, 1, 2.
    (With a jitter other than 0 the alt records' ends move over the breakpoints' bases, and the COV columns with them.)"""
    return _tiled_world(seed, specs, layers, read_len, margin, short, guard, jitter, chrom_prefix, True)


def _tiled_world(seed, specs, layers, read_len, margin, short, guard, jitter, chrom_prefix, ref_guard) -> SynthWorld:
    """make_signature_world (ref_guard False) and make_support_world (True: the guard at the reference breakpoints of every
    haplotype, and the zygosity 'ref')."""
    rng = np.random.default_rng(seed)
    w = SynthWorld()
    for li, (t, span, zyg) in enumerate(specs):
        c = "%s%d" % (chrom_prefix, li + 1)
        t = "TANDUP" if t == "DUP" else t
        span = int(span)
        s0 = margin
        e0 = margin + (span if t != "INS" else 0)       # the event, 0-based half-open
        n = e0 + margin
        ref = w.contigs[c] = random_dna(rng, n)
        ins_seq = random_dna(rng, span) if t == "INS" else None
        # the alt haplotype's segments: (ref start, ref end, strand) or (None, inserted bases, '+')
        if t == "DEL":
            alt = [(0, s0, "+"), (e0, n, "+")]
        elif t == "TANDUP":
            alt = [(0, e0, "+"), (s0, n, "+")]
        elif t == "INV":
            alt = [(0, s0, "+"), (s0, e0, "-"), (e0, n, "+")]
        elif t == "INS":
            alt = [(0, s0, "+"), (None, ins_seq, "+"), (s0, n, "+")]
        else:
            raise ValueError(t)
        plain = [(0, n, "+")]
        haps = [alt, alt] if zyg == "hom" else [plain, plain] if ref_guard and zyg == "ref" else [plain, alt]
        small = span <= short and t != "INV"
        recs = w.reads.setdefault(c, [])
        for h, segs in enumerate(haps):
            # the haplotype's segments in its own coordinates: (hap start, hap end, segment)
            at, table = 0, []
            for sg in segs:
                ln = len(sg[1]) if sg[0] is None else sg[1] - sg[0]
                table.append((at, at + ln, sg))
                at += ln
            m = at
            joints = [p1 for _p0, p1, _sg in table[:-1]]
            if segs is plain:
                zones = []
            elif small:
                zones = [(joints[0] - guard - (span if t == "TANDUP" else 0), joints[-1] + guard + (span if t == "TANDUP" else 0))]
            else:
                zones = [(j - guard, j + guard) for j in joints]
            if ref_guard:
                # (where the haplotype carries a reference breakpoint inside or at an end of a forward segment)
                zones = zones + [(p0 + bp - sg[0] - guard, p0 + bp - sg[0] + guard) for p0, _p1, sg in table
                                 if sg[0] is not None and sg[2] == "+" for bp in (s0, e0) if sg[0] <= bp <= sg[1]]
            for k in range(layers):
                d = int(jitter[k % len(jitter)]) if segs is not plain else 0
                cuts = sorted({0, m} | {x for x in range((k * read_len) // layers, m, read_len) if not any(lo < x < hi for lo, hi in zones)})
                for ri, (a, z) in enumerate(zip(cuts[:-1], cuts[1:])):
                    qname = "%s_h%d_l%d_r%d" % (c, h, k, ri)
                    pieces = []                       # (segment, offset of the piece in it, length)
                    for p0, p1, sg in table:
                        lo, hi = max(a, p0), min(z, p1)
                        if hi > lo:
                            pieces.append((sg, lo - p0, hi - lo))
                    seqs = []
                    for sg, off, ln in pieces:
                        if sg[0] is None:
                            seqs.append(sg[1][off:off + ln])
                        elif sg[2] == "+":
                            seqs.append(ref[sg[0] + off:sg[0] + off + ln])
                        else:
                            seqs.append(revcomp(ref[sg[0]:sg[1]])[off:off + ln])
                    seq = "".join(seqs)
                    if len(pieces) == 1:
                        sg, off, ln = pieces[0]
                        if sg[0] is None:
                            continue                  # (inside a long insertion: not aligned)
                        if sg[2] == "+":
                            recs.append(SamRecord(qname, c, sg[0] + off + 1, "%dM" % ln, seq, ln))
                        else:
                            lo = sg[1] - off - ln
                            recs.append(SamRecord(qname, c, lo + 1, "%dM" % ln, revcomp(seq), ln, flag=0x10))
                        continue
                    if small:
                        # one record: the bases left of the event, the event as one operation, the bases right of it
                        lo = pieces[0][0][0] + pieces[0][1]
                        if t == "DEL":
                            left, right = pieces[0][2], pieces[1][2]
                            cg = "%dM%dD%dM" % (left + d, span, right - d)
                            rspan = left + span + right
                        elif t == "INS":
                            left, right = pieces[0][2], pieces[2][2]
                            cg = "%dM%dI%dM" % (left + d, span, right - d)
                            rspan = left + right
                        else:                         # TANDUP: the first copy is the inserted one (left-aligned)
                            left = s0 - lo
                            right = len(seq) - left - span
                            cg = "%dM%dI%dM" % (left + d, span, right - d)
                            rspan = left + right
                        recs.append(SamRecord(qname, c, lo + 1, cg, seq, rspan))
                        continue
                    # split: a record per aligned piece, the rest of the read soft-clipped; the longest is the primary.  The
                    # jitter moves a breakpoint to the right: the piece left of it d bases longer, the one right of it d shorter
                    aligned = [i for i, pc in enumerate(pieces) if pc[0][0] is not None]
                    main = max(aligned, key=lambda i: (pieces[i][2], -i))
                    for i in aligned:
                        sg, off, ln = pieces[i]
                        before = sum(pc[2] for pc in pieces[:i])
                        after = sum(pc[2] for pc in pieces[i + 1:])
                        gl = -d if before else 0      # the piece's left end in the read moves right by d: it loses d bases there
                        gr = d if after else 0        # ... its right end moves right by d: it gains d bases there
                        before, ln, after = before - gl, ln + gl + gr, after - gr
                        flag = 0 if i == main else 0x800
                        if sg[2] == "+":
                            lo = sg[0] + off - gl
                            cg = ("%dS" % before if before else "") + "%dM" % ln + ("%dS" % after if after else "")
                            recs.append(SamRecord(qname, c, lo + 1, cg, seq, ln, flag=flag))
                        else:
                            # the reverse strand: the read's left end is the record's right end
                            hi = sg[1] - off + gl
                            cg = ("%dS" % after if after else "") + "%dM" % ln + ("%dS" % before if before else "")
                            recs.append(SamRecord(qname, c, hi - ln + 1, cg, revcomp(seq), ln, flag=flag | 0x10))
        recs.sort(key=lambda r: r.pos)
        if t == "INS":
            w.loci.append(Locus(c, t, s0, s0 + 1, "sg%d" % (li + 1), ins_seq))
        else:
            w.loci.append(Locus(c, t, s0 + 1, e0, "sg%d" % (li + 1)))
    return w


LINKS_SPECS = ("DEL", "TANDUP", "INV", "3to5", "3to3")
LINKS_DECOYS = ("no_sa", "other_contig", "off_by_one", "wrong_strand", "low_mapq")
LINKS_DECOY_MAPQ = 3           # the mapQ of the `low_mapq` decoy's entry: a link for --min-mapq 3 and below, nothing above


def make_links_world(seed: int, specs: Sequence[str] = LINKS_SPECS, reads: int = 4, half: int = 500, span: int = 12000,
                     margin: int = 3000, jitter: Sequence[int] = (0,), ref_reads: int = 2, tol: int = 50,
                     decoys: Sequence[str] = LINKS_DECOYS, chrom_prefix: str = "k") -> SynthWorld:
    """A world whose SA tags mean something (`--links`).  Per spec a locus: DEL, TANDUP and INV of `span` bases on
    a contig of their own, the event on bases [margin + 1, margin + span]; '3to5' and '3to3' breakends between two contigs of
    their own, A:p and B:q with p = q = margin.  Every junction of the alt allele is crossed by `reads` molecules of 2 * half
    bases, each written as an aligner writes it - a primary and a supplementary record (0x800), each aligned on its side of the
    junction with the rest soft-clipped and an SA tag that names the other, `rname,pos,strand,CIGAR,60,0;` - molecule k read
    from the forward strand for even k and from the reverse strand for odd k (both records' strand flips, the relation of the two
    does not).  The molecules are those of DESIGN.md 4.21, with the junction's two coordinates x1 < x2 (or A:p and B:q):
      DEL      x1 = J0, x2 = J1:  a piece that ends at J0 (RCLIP) and one that starts at J1 (LCLIP), same strand
      TANDUP   a piece that starts at J0 (LCLIP) and one that ends at J1 (RCLIP), same strand
      INV      the left junction: a piece that ends at J0 and one that ends at J1 (both RCLIP), opposite strands;
               the right junction: a piece that starts at J0 and one that starts at J1 (both LCLIP), opposite strands
      3to5     a piece that ends at A:p (RCLIP) and one that starts at B:q - 1 (LCLIP), same strand
      3to3     a piece that ends at A:p and one that ends at B:q (both RCLIP), opposite strands
    jitter: molecule k reports the first coordinate d = jitter[k % len(jitter)] bases to the right; the second moves with it -
    by d when the two events differ (one piece grows by what the other loses on the same strand), by -d when they are the same
    event.  `ref_reads` unclipped reads cross every breakpoint.  Decoys, one record each per locus, clipped at a breakpoint
    exactly (`decoys` names those planted):
      no_sa         at the left breakpoint, no SA tag                                        (a clip, not a split)
      other_contig  at the left breakpoint, the right entry on a contig named <partner>x      (split, not linked: OL)
      off_by_one    at the left breakpoint, the entry tol + 1 bases off                       (OL)
      wrong_strand  at the right breakpoint, the right place on the other strand              (OR)
      low_mapq      at the right breakpoint, the right entry with mapQ LINKS_DECOY_MAPQ        (a link at offset 0 unless cut)
    For an INV the decoys are planted for the first region of each side.  With these all seven columns are known in closed form:
    L = R = reads (INV: 2 * reads) + what low_mapq adds to R, OL = 2, OR = 1, the offsets the modes of the jitter."""
    from . import links as _links
    rng = np.random.default_rng(seed)
    w = SynthWorld()
    h = int(half)

    def piece(c, x, ev, m):
        """(pos0, CIGAR without its clip side filled in) of a piece of m aligned bases with event ev at x"""
        return (x - m, x) if ev == _links.RCLIP else (x, x + m)

    def record(qname, c, x, ev, m, clip_seq, flag, sa, mapq=60):
        lo, hi = piece(c, x, ev, m)
        own = w.contigs[c][lo:hi]
        s = len(clip_seq)
        if ev == _links.RCLIP:
            cg, seq = "%dM%dS" % (m, s), own + clip_seq
        else:
            cg, seq = "%dS%dM" % (s, m), clip_seq + own
        w.reads.setdefault(c, []).append(SamRecord(qname, c, lo + 1, cg, seq, m, {"SA": sa} if sa is not None else None, flag, mapq))

    def entry(c, x, ev, m, s, minus, mapq=60):
        lo, _hi = piece(c, x, ev, m)
        cg = "%dM%dS" % (m, s) if ev == _links.RCLIP else "%dS%dM" % (s, m)
        return "%s,%d,%s,%s,%d,0;" % (c, lo + 1, "-" if minus else "+", cg, mapq)

    def molecule(qname, c1, x1, ev1, c2, x2, ev2, other, d, flip):
        """the two records of a molecule whose pieces have (ev1 at x1 + d) and (ev2 at x2 + d or x2 - d)"""
        d2 = d if ev1 != ev2 else -d
        m1 = h + d if ev1 == _links.RCLIP else h - d
        m2 = 2 * h - m1
        f1, f2 = (0x10 if flip else 0), (0x10 if flip != other else 0)
        lo1, hi1 = piece(c1, x1 + d, ev1, m1)
        lo2, hi2 = piece(c2, x2 + d2, ev2, m2)
        s1, s2 = w.contigs[c1][lo1:hi1], w.contigs[c2][lo2:hi2]
        record(qname, c1, x1 + d, ev1, m1, revcomp(s2) if other else s2, f1, entry(c2, x2 + d2, ev2, m2, m1, bool(f2)))
        record(qname, c2, x2 + d2, ev2, m2, revcomp(s1) if other else s1, f2 | 0x800, entry(c1, x1 + d, ev1, m1, m2, bool(f1)))

    for li, t in enumerate(specs):
        tag = "%s%d" % (chrom_prefix, li + 1)
        if t in ("DEL", "TANDUP", "INV"):
            c = tag
            n = 2 * margin + span
            w.contigs[c] = random_dna(rng, n)
            j0, j1 = margin, margin + span
            locus = [c, j0 + 1, j1]
            w.loci.append(Locus(c, t, j0 + 1, j1, "lk%d" % (li + 1)))
            if t == "DEL":
                juncs = [(c, j0, _links.RCLIP, c, j1, _links.LCLIP, False)]
            elif t == "TANDUP":
                juncs = [(c, j0, _links.LCLIP, c, j1, _links.RCLIP, False)]
            else:
                juncs = [(c, j0, _links.RCLIP, c, j1, _links.RCLIP, True), (c, j0, _links.LCLIP, c, j1, _links.LCLIP, True)]
            points = [(c, j0), (c, j1)]
        elif t in ("3to5", "3to3"):
            ca, cb = tag + "a", tag + "b"
            p = q = margin
            w.contigs[ca] = random_dna(rng, 2 * margin)
            w.contigs[cb] = random_dna(rng, 2 * margin)
            locus = [ca, p, cb, q, t, ""]
            w.loci.append(Locus(ca, "BND", p, q, "lk%d" % (li + 1), "", {"form": t, "mate_chrom": cb}))
            if t == "3to5":
                juncs = [(ca, p, _links.RCLIP, cb, q - 1, _links.LCLIP, False)]
            else:
                juncs = [(ca, p, _links.RCLIP, cb, q, _links.RCLIP, True)]
            points = [(ca, p), (cb, q)]
        else:
            raise ValueError(t)
        for ji, (c1, x1, ev1, c2, x2, ev2, other) in enumerate(juncs):
            for k in range(reads):
                molecule("%s_j%d_m%d" % (tag, ji, k), c1, x1, ev1, c2, x2, ev2, other, int(jitter[k % len(jitter)]), bool(k & 1))
        for c, x in points:
            for k in range(ref_reads):
                lo = x - h + 37 * (k + 1)
                w.reads.setdefault(c, []).append(SamRecord("%s_ref%d_%d" % (tag, x, k), c, lo + 1, "%dM" % (2 * h), w.contigs[c][lo:lo + 2 * h], 2 * h))
        # the decoys: the question of the side's first region, answered wrongly in one way each
        left, right = _links.regions("BND" if t in ("3to5", "3to3") else t, locus, lambda name: len(w.contigs[name]))
        for name in decoys:
            c, f, pc = (left if name in ("no_sa", "other_contig", "off_by_one") else right)[0]
            x, y, ev, pend, rel = f[2], f[3], f[6], f[7], f[8]
            clip = random_dna(rng, h)
            minus = bool(rel)                      # the record is on the forward strand: the entry's strand by the relation
            if name == "no_sa":
                sa = None
            else:
                yy = y + tol + 1 if name == "off_by_one" else y
                sa = entry(pc + "x" if name == "other_contig" else pc, yy, _links.RCLIP if pend == _links.END_B else _links.LCLIP, h, h,
                           (not minus) if name == "wrong_strand" else minus, LINKS_DECOY_MAPQ if name == "low_mapq" else 60)
            record("%s_decoy_%s" % (tag, name), c, x, ev, h, clip, 0, sa)
    for c in w.reads:
        w.reads[c].sort(key=lambda r: r.pos)
    return w


def links_vcf_text(world: SynthWorld) -> str:
    """make_links_world's loci as `vapor vcf --bnd` reads them: the DEL, TANDUP and INV records of vcf_text, then the breakend
    records of bnd_vcf_text with their mates."""
    simple = SynthWorld()
    simple.loci = [l for l in world.loci if l.svtype != "BND"]
    return vcf_text(simple) + bnd_vcf_text(world, True)


def mirror_world(world: SynthWorld) -> SynthWorld:
    """M(W): the world as its reverse-complemented contigs hold it (x -> L + 1 - x on a contig of L bases; `--both-ends`,
    DESIGN.md 4.14).  Contigs: their reverse complement (seqio.rc_read: nothing is dropped).  Records: seqio.mirror_records -
    POS = L + 1 - the alignment's last reference base, the CIGAR operations reversed, rc(SEQ), tags kept - sorted by the new POS
    (stable).  Loci: DEL / INV / TANDUP / INS at (L + 1 - end, L + 1 - start); a breakend at (La + 1 - p, Lb + 1 - q) in the form
    the junction has on the other strand (3to5 <-> 5to3, 3to3 <-> 5to5), its inserted bases reverse complemented.  The contigs
    must be text (a world of virtual contigs is not mirrored)."""
    from . import seqio
    m = SynthWorld()
    for c, seq in world.contigs.items():
        if not isinstance(seq, str):
            raise TypeError("mirror_world: contig %s is not text" % c)
        m.contigs[c] = seqio.rc_read(seq)
    for c, recs in world.reads.items():
        n = len(world.contigs[c])
        out = []
        for r, (q, pos, cig, seq) in zip(recs, seqio.mirror_records([(r.qname, r.pos, r.cigar, r.seq) for r in recs], n)):
            span = sum(int(k) for k, op in seqio._CIGAR_RE.findall(cig) if op in "M=D")
            out.append(SamRecord(q, c, pos, cig, seq, span, dict(r.tags) if r.tags else None))
        out.sort(key=lambda r: r.pos)
        m.reads[c] = out
    other = {"3to5": "5to3", "5to3": "3to5", "3to3": "5to5", "5to5": "3to3"}
    for l in world.loci:
        n = len(world.contigs[l.chrom])
        if l.svtype == "BND":
            nb = len(world.contigs[l.extra["mate_chrom"]])
            m.loci.append(Locus(l.chrom, "BND", n + 1 - l.start, nb + 1 - l.end, l.svid, seqio.rc_read(l.ins_seq or ""),
                                {"form": other[l.extra["form"]], "mate_chrom": l.extra["mate_chrom"]}))
        else:
            m.loci.append(Locus(l.chrom, l.svtype, n + 1 - l.end, n + 1 - l.start, l.svid,
                                seqio.rc_read(l.ins_seq) if l.ins_seq else l.ins_seq, dict(l.extra) if l.extra else None))
    return m


def bnd_records(world: SynthWorld, mates: bool = True) -> List[List[str]]:
    """VCF records (lists of the ten columns) of make_bnd_world's junctions: the record at A:p, then its mate at B:q, paired by
    ID / MATEID."""
    mate_form = {"3to5": "5to3", "3to3": "3to3", "5to3": "3to5", "5to5": "5to5"}
    out = []
    for l in world.loci:
        if l.svtype != "BND":
            continue
        form, cb, p, q, I = l.extra["form"], l.extra["mate_chrom"], l.start, l.end, l.ins_seq or ""
        ra, rb = world.contigs[l.chrom][p - 1], world.contigs[cb][q - 1]
        i1, i2 = l.svid + "_1", l.svid + "_2"
        out.append([l.chrom, str(p), i1, ra, bnd_alt(form, ra, I, cb, q), ".", "PASS",
                    "SVTYPE=BND" + (";MATEID=" + i2 if mates else ""), "GT", "0/1"])
        if mates:
            mi = I if form in ("3to5", "5to3") else revcomp(I)
            out.append([cb, str(q), i2, rb, bnd_alt(mate_form[form], rb, mi, l.chrom, p), ".", "PASS", "SVTYPE=BND;MATEID=" + i1,
                        "GT", "0/1"])
    return out


def bnd_vcf_text(world: SynthWorld, mates: bool = True, header: bool = False) -> str:
    out = ["##fileformat=VCFv4.2", "##source=vapor_amd.synth",
           "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE"] if header else []
    out += ["\t".join(r) for r in bnd_records(world, mates)]
    return "\n".join(out) + "\n"


def complex_vcf_text(world: SynthWorld, header: bool = False) -> str:
    """VCF records for make_complex_world's loci with the INFO keys vapor_vali/vapor:87-125, 176-202 read:
    insert_point=chrom:pos (DISDUP, DUP_INV), del=/inv= (DEL_INV), Other=ref_alt_chrom:bp:bp:bp."""
    out = ["##fileformat=VCFv4.1", "##source=vapor_amd.synth",
           "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE"] if header else []
    for l in world.loci:
        if l.svtype in ("DISDUP", "DUP_INV"):
            info = "SVTYPE=%s;END=%d;insert_point=%s:%d" % (l.svtype, l.end, l.extra["insert_chrom"], l.extra["insert_point"])
        elif l.svtype == "DEL_INV":
            info = "SVTYPE=DEL_INV;END=%d;" % l.end + ";".join("%s=%s:%d-%d" % (k, l.chrom, x0, x1) for x0, x1, k in l.extra["blocks"])
        elif l.svtype == "OTHER":
            r, a = l.extra["other"]
            info = "SVTYPE=CPLX;END=%d;Other=%s_%s_%s:%s" % (l.end, r, a, l.chrom, ":".join(str(x) for x in l.extra["bps"]))
        else:
            raise ValueError(l.svtype)
        out.append("\t".join([l.chrom, str(l.start), l.svid, "N", "<%s>" % l.svtype, ".", "PASS", info, "GT", "0/1"]))
    return "\n".join(out) + "\n"


def phase_world(world: SynthWorld, seed: int, untagged: float = 0.2, phase_set: int = 1) -> SynthWorld:
    """Haplotag an existing world in place (make_world's own draws are not touched): the loci in world.loci order, inside a
    locus one rng.random() per read of world.reads[chrom], in list order, from default_rng(seed).  A draw below `untagged`
    leaves the read untagged; otherwise a read whose name ends in 'a' (drawn from the alt haplotype) gets HP = 1, any other
    HP = 2, and PS = phase_set.  (A contig that several loci share is walked once per locus; the last walk decides.)"""
    rng = np.random.default_rng(seed)
    for l in world.loci:
        for r in world.reads.get(l.chrom, ()):
            if rng.random() < untagged:
                r.tags = None
            else:
                r.tags = {"HP": 1 if r.qname.endswith("a") else 2, "PS": int(phase_set)}
    return world


DECOY_MARKS = ("mapq0", "mapq_low", "unmapped", "secondary", "qcfail", "duplicate", "supplementary")


def add_decoys(world: SynthWorld, seed: int, per_contig: int = 7, min_mapq: int = 20, marks: Sequence[str] = DECOY_MARKS,
               errors: Tuple[float, float, float] = (0.01, 0.08, 0.04), stoppers: int = 0) -> SynthWorld:
    """A copy of `world` with decoy records planted between its own (the read filter's worlds; `world` itself, its
    records and make_world's draws are not touched - the copy shares contigs, loci and record objects).  Per contig that has
    reads, `per_contig` decoys from default_rng(seed): decoy i takes record R = recs[i * len(recs) // per_contig] as its template -
    it starts where R's bases start on the contig (POS minus a leading soft clip) and is as long as R's SEQ, so it lies before the
    same windows with as many bases behind them - and its bases come from the OTHER allele: the contig itself (a reference read)
    where R's name ends in 'a', the alternative haplotype (apply_sv of the contig's one DEL / TANDUP / INV / INS locus) where it
    ends in 'r'; a template whose other allele cannot be made (a reference read on a contig of breakends) is passed over.  The
    decoy follows R in the list, named d<i>_<R's name> with the last letter that of its own allele, and carries mark marks[i % len(marks)]:

        mapq0          MAPQ 0                              qcfail         FLAG 0x200
        mapq_low       MAPQ min_mapq - 1                   duplicate      FLAG 0x400
        unmapped       FLAG 0x4, CIGAR '*' (no operation)  supplementary  FLAG 0x800
        secondary      FLAG 0x100, SEQ '' (l_seq 0)

    Every other field is MAPQ 60, FLAG 0.  Five of the marks sit on records today's rule keeps: they vote.  The unmapped mate and
    the secondary record without SEQ lie where today's rule passes them over (a mate without CIGAR stops a region only when its
    POS is the window start itself).  `--min-mapq min_mapq --exclude-flags 0xF04` filters every decoy and nothing else; 0x904 does
    when `marks` leaves out qcfail and duplicate.  `stoppers`: on the first that many contigs of one DEL / INV / TANDUP locus the
    unmapped decoy is placed ON the start of the locus's read window (SV start minus min(500, span), SF:794-802) instead: there
    it reaches the CIGAR walk, and without the filter the whole run ends in the reference's IndexError (SF:331).  A tagged template (phase_world) hands the decoy HP of its own allele and R's PS."""
    import re
    rng = np.random.default_rng(seed)
    out = SynthWorld()
    out.contigs, out.loci = world.contigs, world.loci
    for attr in ("cache_ok",):
        if hasattr(world, attr):
            setattr(out, attr, getattr(world, attr))
    simple = {}
    for l in world.loci:
        if l.svtype in ("DEL", "TANDUP", "DUP", "INV", "INS"):
            simple.setdefault(l.chrom, []).append(l)
    for c, recs in world.reads.items():
        ref = world.contigs[c]
        alt = None
        if len(simple.get(c, ())) == 1:
            l = simple[c][0]
            alt = apply_sv(ref, l.svtype, l.start, l.end, l.ins_seq)
        new = list(recs)
        planted = 0
        stop_at = None
        if stoppers > 0 and len(simple.get(c, ())) == 1 and simple[c][0].svtype in ("DEL", "TANDUP", "DUP", "INV") and recs:
            l = simple[c][0]
            stop_at = l.start - min(500, l.end - l.start)
            stoppers -= 1
        for i in range(per_contig if recs else 0):
            at = i * len(recs) // per_contig
            R = recs[at]
            hap = ref if R.qname.endswith("a") else alt
            if hap is None:
                continue
            m = re.match(r"(\d+)S", R.cigar)
            a = max(R.pos - 1 - (int(m.group(1)) if m else 0), 0)
            b = min(a + max(len(R.seq), 1), len(hap))
            read, cigar = mutate(rng, hap[a:b], *errors)
            mark = marks[i % len(marks)]
            d = SamRecord("d%d_" % i + R.qname[:-1] + ("r" if hap is ref else "a"), c, a + 1, cigar, read, b - a)
            if R.tags:
                d.tags = {"HP": 2 if hap is ref else 1, "PS": R.tags.get("PS", 1)}
            if mark == "mapq0":
                d.mapq = 0
            elif mark == "mapq_low":
                d.mapq = max(int(min_mapq) - 1, 0)
            elif mark == "unmapped":
                d.flag, d.cigar, d.ref_span = 0x4, "*", 1
                if stop_at is not None and stop_at >= 1:
                    d.pos = stop_at
            elif mark == "secondary":
                d.flag, d.seq = 0x100, ""
            elif mark in ("qcfail", "duplicate", "supplementary"):
                d.flag = {"qcfail": 0x200, "duplicate": 0x400, "supplementary": 0x800}[mark]
            else:
                raise ValueError("add_decoys: unknown mark %r" % (mark,))
            new.insert(at + 1 + planted, d)
            planted += 1
        out.reads[c] = new
    return out


def add_split_alignments(world: SynthWorld, variant: str = "full", window_dups: int = 2) -> SynthWorld:
    """A copy of `world` in which a molecule that crosses a junction is written the way an aligner reports it: several records
    with one QNAME (the worlds of `--dedup-qname`; `world` itself and its records are not touched - the copy
    shares contigs, loci and the records it does not add).  For the loci whose two pieces lie on forward strands - DEL and
    TANDUP of make_junction_world, 3to5 breakends without inserted bases of make_bnd_world - every alt-allele read that is
    aligned up to the junction and soft-clipped after it (xM yS, the primary record, FLAG 0) gets a supplementary record (FLAG
    0x800, MAPQ and tags of the primary) with the same QNAME at the far breakpoint, S then M: the clipped bases aligned from
    there on as one M operation.  variant:

        'full'  the supplementary carries the whole SEQ, xS yM (minimap2 -Y): the right-anchored view of the far breakpoint keeps
                it, so the molecule is in two views of `--both-ends`
        'hard'  it is hard-clipped, xH yM, SEQ the y bases alone: too short for any window of 2 * 500 bases, no view keeps it

    window_dups: on every TANDUP contig the first that many primary records also get a twin inside the same window - FLAG 0x100
    (secondary), the same QNAME, SEQ and CIGAR, five bases further right - which today's rule keeps beside the primary.
    `planted` on the copy counts what was added: {'split': n, 'window': m}."""
    import re
    if variant not in ("full", "hard"):
        raise ValueError("add_split_alignments: variant %r" % (variant,))
    out = SynthWorld()
    out.contigs, out.loci = world.contigs, world.loci
    if hasattr(world, "cache_ok"):
        out.cache_ok = world.cache_ok
    out.reads = {c: list(rs) for c, rs in world.reads.items()}
    out.planted = {"split": 0, "window": 0}
    for l in world.loci:
        if l.svtype == "DEL":
            near, far_c, far_at = l.start, l.chrom, l.end + 1
        elif l.svtype == "TANDUP":
            near, far_c, far_at = l.end, l.chrom, l.start + 1
        elif l.svtype == "BND" and (l.extra or {}).get("form") == "3to5" and not l.ins_seq:
            near, far_c, far_at = l.start, l.extra["mate_chrom"], l.end
        else:
            continue
        dups = window_dups if l.svtype == "TANDUP" else 0
        for r in world.reads.get(l.chrom, ()):
            m = re.fullmatch(r"(.*[MIDN=X])(\d+)S", r.cigar)
            if m is None or r.flag != 0 or r.pos - 1 + r.ref_span != near:
                continue
            y = int(m.group(2))
            x = len(r.seq) - y
            if x < 1 or y < 1:
                continue
            sup = SamRecord(r.qname, far_c, far_at, ("%dS%dM" if variant == "full" else "%dH%dM") % (x, y),
                            r.seq if variant == "full" else r.seq[x:], y, dict(r.tags) if r.tags else None, 0x800, r.mapq)
            out.reads.setdefault(far_c, []).append(sup)
            out.planted["split"] += 1
            if dups > 0:
                out.reads[l.chrom].append(SamRecord(r.qname, r.rname, r.pos + 5, r.cigar, r.seq, r.ref_span,
                                                    dict(r.tags) if r.tags else None, 0x100, r.mapq))
                out.planted["window"] += 1
                dups -= 1
    for rs in out.reads.values():
        rs.sort(key=lambda r: r.pos)            # (stable: a planted record follows the records of its position)
    return out


def snv_world(world: SynthWorld, seed: int, spacing: int = 40) -> dict:
    """Plant phased heterozygous SNVs into an existing world in place (make_world's own draws are not touched; do it before a
    backend has seen the world - the reads' SEQ strings are replaced).  From default_rng(seed), the loci in world.loci order: the
    sites of a locus lie left of its SV start - the reads' CIGARs are relative to their own haplotype, and only there do both
    haplotypes share the reference's coordinates - at 1-based positions that step by `spacing` with a jitter of a quarter of it
    either way; per site a random other base as ALT and a random `1|0` or `0|1`.  Then, per read of the locus's contig and
    per site its CIGAR covers with M, the read's base is overwritten with its haplotype's allele (a name ending in 'a' is
    haplotype 1, any other haplotype 2) where it still equals the reference base - so the read's own substitution errors at
    sites survive.  Returns {contig: [(pos, REF, ALT, GT), ...]} in position order (snv_vcf_text writes it)."""
    import re
    rng = np.random.default_rng(seed)
    ops_re = re.compile(r"(\d+)([MIDNSHP=X])")
    out: dict = {}
    jit = max(spacing // 4, 1)
    for l in world.loci:
        ref = world.contigs[l.chrom]
        sites = []
        p = 1 + int(rng.integers(1, spacing + 1))
        while p <= l.start:
            r = ref[p - 1]
            alt = [c for c in "ACGT" if c != r][int(rng.integers(0, 3))]
            sites.append((p, r, alt, "1|0" if rng.random() < 0.5 else "0|1"))
            p += spacing + int(rng.integers(-jit, jit + 1))
        out[l.chrom] = sites
        for rec in world.reads.get(l.chrom, ()):
            h = 0 if rec.qname.endswith("a") else 1
            seq = None
            rr, q, si = rec.pos, 0, 0
            for m in ops_re.finditer(rec.cigar):              # (lazily: the sites end left of the SV, a few operations in)
                n, op = int(m.group(1)), m.group(2)
                if op == "M":
                    while si < len(sites) and sites[si][0] < rr:
                        si += 1
                    while si < len(sites) and sites[si][0] < rr + n:
                        pos, r, alt, gt = sites[si]
                        qi = q + pos - rr
                        allele = alt if gt.split("|")[h] == "1" else r
                        if qi < len(rec.seq) and rec.seq[qi] == r and allele != r:
                            if seq is None:
                                seq = bytearray(rec.seq.encode("ascii"))
                            seq[qi] = ord(allele)
                        si += 1
                    rr += n
                    q += n
                elif op == "I":
                    q += n
                elif op == "D":
                    rr += n
                if si >= len(sites):
                    break
            if seq is not None:
                rec.seq = seq.decode("ascii")
    return out


def snv_vcf_text(sites: dict, sample: str = "S1", phase_set: int = 1) -> str:
    """snv_world's sites as a phased VCF of one sample: GT:PS per record, every site in phase set `phase_set`."""
    out = ["##fileformat=VCFv4.2", "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">",
           "##FORMAT=<ID=PS,Number=1,Type=Integer,Description=\"Phase set\">", "##source=vapor_amd.synth",
           "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + sample]
    for chrom, rows in sites.items():
        for pos, r, alt, gt in rows:
            out.append("\t".join([chrom, str(pos), ".", r, alt, ".", "PASS", ".", "GT:PS", "%s:%d" % (gt, phase_set)]))
    return "\n".join(out) + "\n"


def write_world_files(world: SynthWorld, directory: str, block_size: int = 8192, qual_seed=None,
                      bgzip_reference: bool = False) -> Tuple[str, str]:
    """FASTA + .fai and coordinate-sorted BAM + .bai of a synthetic world, written by this package alone
    (vapor_amd.bamio); returns (fasta path, bam path).  Reads keep their order inside one start position.  With
    `bgzip_reference` the reference is written bgzipped instead (ref.fa.gz + .fai + .gzi, seqio.write_bgzf_fasta)."""
    import os
    from . import bamio
    names = list(world.contigs)
    if bgzip_reference:
        from . import seqio
        fa = seqio.write_bgzf_fasta(os.path.join(directory, "ref.fa.gz"),
                                    [(n, world.contigs[n] if isinstance(world.contigs[n], str) else world.contigs[n][0:len(world.contigs[n])])
                                     for n in names])
    else:
        fa = os.path.join(directory, "ref.fa")
        _write_plain_fasta(world, fa, names)
    recs = [(r.qname, names.index(c), r.pos - 1, r.cigar, r.seq, r.tags, r.mapq, r.flag) for c, rs in world.reads.items() for r in rs]
    bam = os.path.join(directory, "reads.bam")
    bamio.write_bam(bam, [(n, len(world.contigs[n])) for n in names], recs, block_size=block_size, qual_seed=qual_seed)
    return fa, bam


def _write_plain_fasta(world, fa, names):
    with open(fa, "w") as f, open(fa + ".fai", "w") as fi:
        off = 0
        for n in names:
            seq = world.contigs[n]
            seq = seq[0:len(seq)] if not isinstance(seq, str) else seq
            hdr = ">" + n + "\n"
            f.write(hdr)
            off += len(hdr)
            fi.write("%s\t%d\t%d\t60\t61\n" % (n, len(seq), off))
            for i in range(0, len(seq), 60):
                f.write(seq[i:i + 60] + "\n")
            off += len(seq) + (len(seq) + 59) // 60


# ---------------------------------------------------------------------------
# at-size worlds of DISTINCT loci without holding them: tiles of a base world, every tile mutated on its own
# ---------------------------------------------------------------------------
_NEXT_BASE = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"CGTAcgta"):
    _NEXT_BASE[_a] = _b


def _mutated(text: str, rng, rate: float = 0.002) -> str:
    """`text` with one base in five hundred replaced by the next one of A -> C -> G -> T -> A (case kept, other symbols
    kept): another sequence of the same length and structure."""
    a = np.frombuffer(text.encode("ascii"), dtype=np.uint8).copy()
    if len(a):
        pos = rng.integers(0, len(a), size=max(1, int(len(a) * rate)))
        a[pos] = _NEXT_BASE[a[pos]]
    return a.tobytes().decode("ascii")


class _LazyTiles:
    """Mapping `<base name>.t<k>` -> the base world's entry, mutated for tile k when it is asked for; the last `cap` answers are
    kept (a chunk's loci are neighbours).  Stands in for SynthWorld.contigs / .reads."""

    def __init__(self, base: dict, n_tiles: int, make, cap: int):
        from collections import OrderedDict
        self.base, self.n_tiles, self.make, self.cap = base, n_tiles, make, cap
        self.lru = OrderedDict()
        import threading
        self.lock = threading.Lock()
        self.made = 0
        self.seconds = 0.0

    def _split(self, name):
        b, _, k = name.rpartition(".t")
        return (b, int(k)) if b in self.base and k.isdigit() and int(k) < self.n_tiles else (None, -1)

    def __contains__(self, name):
        return self._split(name)[0] is not None

    def __getitem__(self, name):
        with self.lock:
            got = self.lru.get(name)
            if got is not None:
                self.lru.move_to_end(name)
                return got
        b, k = self._split(name)
        if b is None:
            raise KeyError(name)
        import time
        t0 = time.perf_counter()
        got = self.make(b, k)
        with self.lock:
            self.seconds += time.perf_counter() - t0
            self.made += 1
            self.lru[name] = got
            while len(self.lru) > self.cap:
                self.lru.popitem(last=False)
        return got

    def get(self, name, default=None):
        try:
            return self[name]
        except KeyError:
            return default

    def __len__(self):
        return len(self.base) * self.n_tiles


class DistinctTilesWorld(SynthWorld):
    """`n_tiles` copies of a base world under the contig names `<c>.t<k>`, every copy with its own substitutions in contigs,
    reads and insertion payloads (seeded by tile and contig): as many DISTINCT loci as records, generated when a locus is
    reached and dropped again, so that a 50 000-locus world of 30 kb reads never lies in memory (BASELINE configs[3], [4])."""
    cache_ok = False                   # (backends must not keep per-contig caches of this world: they would keep the world)

    def __init__(self, base: SynthWorld, n_tiles: int, seed: int, cap: int = 1024):
        super().__init__()
        import zlib
        self.base_world, self.n_tiles, self.seed = base, n_tiles, seed

        def rng_of(name, k, what):
            return np.random.default_rng([seed, k, zlib.crc32(name.encode()), what])

        def contig(b, k):
            return _mutated(base.contigs[b], rng_of(b, k, 0))

        def reads(b, k):
            rng = rng_of(b, k, 1)
            return [SamRecord(r.qname, "%s.t%d" % (r.rname, k), r.pos, r.cigar, _mutated(r.seq, rng), r.ref_span) for r in base.reads.get(b, [])]
        self.contigs = _LazyTiles(base.contigs, n_tiles, contig, cap)
        self.reads = _LazyTiles(base.reads, n_tiles, reads, cap)
        self._rng_of = rng_of

    def tile_locus(self, l: Locus, k: int) -> Locus:
        extra = dict(l.extra) if l.extra else None
        if extra and "insert_chrom" in extra:
            extra["insert_chrom"] = "%s.t%d" % (extra["insert_chrom"], k)
        ins = _mutated(l.ins_seq, self._rng_of(l.chrom, k, 2)) if l.ins_seq and "X" not in l.ins_seq else l.ins_seq
        return Locus("%s.t%d" % (l.chrom, k), l.svtype, l.start, l.end, "%s.t%d" % (l.svid, k), ins, extra)

    def fai_rows(self):
        return [("%s.t%d" % (c, k), len(v)) for k in range(self.n_tiles) for c, v in self.base_world.contigs.items()]

"""Haplotype-resolved validation (`vapor bed | vcf --phased`; not in the reference: DESIGN.md §4.13).

A haplotagged BAM carries `HP:i:1|2` and a phase set `PS:i:n` on its alignments.  This module holds the one statement of what
those tags mean here - the tag rule (`tags_from_aux`, `tags_from_sam`), the groups of a locus (`select`), the phased genotype
(`allele`, `quality`) and the nine columns (`columns`) - for the three readers (bamio's Python reader, the library's
vapor_bam_chop_tagged, SAM text), the drivers and the writer.

`--phase-vcf` makes the same (hap, ps) for a BAM that is not haplotagged, from the phased heterozygous SNVs
of a VCF: `read_sites` and `haplotag` are the statement of that rule, for the same three readers (vapor_bam_chop_haplotag in
the library) and for the device's bam_haplotag_kernel.
"""
from __future__ import annotations

import struct
from typing import List, Optional

import numpy as np

INFO = (
    ("VaPoR_PS", "Integer", "1", "Phase set (PS tag) of the haplotagged reads the haplotype columns were taken from (--phased)"),
    ("VaPoR_PGT", "String", "1", "Phased genotype a1|a2: whether most reads of haplotype 1 / haplotype 2 support the prediction (--phased)"),
    ("VaPoR_PGQ", "Float", "1", "Quality of the phased genotype: the smaller log10 likelihood ratio of the two called alleles (--phased)"),
    ("VaPoR_H1_QS", "Float", "1", "VaPoR_QS of the reads of haplotype 1 (--phased)"),
    ("VaPoR_H1_GS", "Float", "1", "VaPoR_GS of the reads of haplotype 1 (--phased)"),
    ("VaPoR_H1_Rec", "Float", ".", "Similarity scores of the reads of haplotype 1 (--phased)"),
    ("VaPoR_H2_QS", "Float", "1", "VaPoR_QS of the reads of haplotype 2 (--phased)"),
    ("VaPoR_H2_GS", "Float", "1", "VaPoR_GS of the reads of haplotype 2 (--phased)"),
    ("VaPoR_H2_Rec", "Float", ".", "Similarity scores of the reads of haplotype 2 (--phased)"),
)
COLUMNS = tuple(i[0] for i in INFO)
PS_NONE = -(1 << 63)          # "no PS field" where a phase set travels as an int64 (vapor_bam_chop_tagged's meta)
PHASE_REACH = 100000          # `--phase-vcf`: a locus's sites lie within this many bases of its region (VAPOR_PHASE_REACH in the header)
PHASE_SETS_DEVICE = 64        # ... and a region with more distinct phase sets among them takes the host route

_AUX_SIZE = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
_AUX_INT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}


# ---------------------------------------------------------------------------------------------
# the tags of a record
# ---------------------------------------------------------------------------------------------
def _hap(v: Optional[int]) -> int:
    return int(v) if v in (1, 2) else 0


def tags_from_aux(rec: bytes, p: int):
    """(hap, ps) of a BAM record whose aux fields start at byte p: hap = the value of the first HP field of integer type
    (c C s S i I) if it is 1 or 2, else 0; ps = the value of the first PS field of integer type, None without one.  The walk is
    find_cg's (vapor_bam.cpp): fixed-size fields by their size, Z / H to their NUL, B arrays by arithmetic; it ends where both
    are found, at the end of the record, or at the first field that is malformed (an unknown type, a field or string that runs
    past the record) - what was found before that point stands."""
    n = len(rec)
    hp = ps = None
    while p + 3 <= n and (hp is None or ps is None):
        t0, t1, typ = rec[p], rec[p + 1], chr(rec[p + 2])
        p += 3
        sz = _AUX_SIZE.get(typ)
        if sz is not None:
            if sz > n - p:
                break
            fmt = _AUX_INT.get(typ)
            if fmt is not None:
                if t0 == 72 and t1 == 80 and hp is None:          # HP
                    hp = struct.unpack_from(fmt, rec, p)[0]
                elif t0 == 80 and t1 == 83 and ps is None:        # PS
                    ps = struct.unpack_from(fmt, rec, p)[0]
            p += sz
        elif typ in "ZH":
            e = rec.find(b"\x00", p)
            if e < 0:
                break
            p = e + 1
        elif typ == "B":
            if p + 5 > n:
                break
            sub, cnt = chr(rec[p]), struct.unpack_from("<i", rec, p + 1)[0]
            p += 5
            es = 1 if sub in "cC" else 2 if sub in "sS" else 4
            if cnt < 0 or cnt * es > n - p:
                break
            p += cnt * es
        else:
            break
    return _hap(hp), ps


def tags_from_sam(fields) -> tuple:
    """The same from the optional fields of a SAM line (`TAG:TYPE:VALUE` strings; SAM text writes every integer type as `i`)."""
    hp = ps = None
    for f in fields:
        if len(f) > 5 and f[2] == ":" and f[3:5] == "i:":
            if hp is None and f[:2] == "HP":
                hp = int(f[5:])
            elif ps is None and f[:2] == "PS":
                ps = int(f[5:])
            if hp is not None and ps is not None:
                break
    return _hap(hp), ps


def _typed(v):
    """(type letter, value) of a tag dict's value: (type, value) as given, an int as i (I above 2^31 - 1), a float as f, a str
    as Z; a B array is ('B', subtype letter, values)."""
    if isinstance(v, tuple):
        return v
    if isinstance(v, (int, np.integer)):
        return ("I" if int(v) > 0x7FFFFFFF else "i", int(v))
    if isinstance(v, float):
        return ("f", v)
    return ("Z", str(v))


def encode_aux(tags: dict) -> bytes:
    """A tag dict as BAM aux bytes, in the dict's order."""
    out = []
    for name, v in tags.items():
        t = _typed(v)
        head = name.encode("ascii")[:2] + t[0].encode("ascii")
        if t[0] == "B":
            fmt = _AUX_INT.get(t[1], "<f")
            out.append(head + t[1].encode("ascii") + struct.pack("<i", len(t[2])) + b"".join(struct.pack(fmt, x) for x in t[2]))
        elif t[0] in "ZH":
            out.append(head + str(t[1]).encode("ascii") + b"\x00")
        elif t[0] == "A":
            out.append(head + str(t[1]).encode("ascii")[:1])
        else:
            out.append(head + struct.pack(_AUX_INT.get(t[0], "<f"), t[1]))
    return b"".join(out)


def sam_fields(tags: dict) -> List[str]:
    """The same dict as the optional fields of a SAM line (every integer type reads `i` there)."""
    out = []
    for name, v in tags.items():
        t = _typed(v)
        if t[0] == "B":
            out.append("%s:B:%s,%s" % (name, t[1], ",".join(str(x) for x in t[2])))
        elif t[0] in _AUX_INT:
            out.append("%s:i:%d" % (name, t[1]))
        else:
            out.append("%s:%s:%s" % (name, t[0], t[1]))
    return out


# ---------------------------------------------------------------------------------------------
# haplotags from a phased VCF (`--phase-vcf`): the sites, the vote of a record, its tag
# ---------------------------------------------------------------------------------------------
_NT16 = "=ACMGRSVTWYHKDBN"                       # BAM's 4-bit alphabet: A C G T are 1 2 4 8
_CIGAR_OPS = "MIDNSHP=X"
_CIGAR_TEXT = None


class Sites:
    """The phased heterozygous SNVs of one sample: per contig four arrays in position order - pos (int64, 1-based), a1 and a2
    (uint8: what haplotype 1 / 2 carries, as BAM 4-bit codes), ps (int64)."""

    def __init__(self, by_contig: dict):
        self.by_contig = by_contig

    def __len__(self) -> int:
        return sum(len(v[0]) for v in self.by_contig.values())

    def of(self, chrom: str, start: int, end: int):
        """The sites of a locus whose region is [start, end]: those of its contig with start - PHASE_REACH <= pos <= end +
        PHASE_REACH, as (pos, a1, a2, ps) arrays; None without any."""
        v = self.by_contig.get(chrom)
        if v is None:
            return None
        a = int(np.searchsorted(v[0], int(start) - PHASE_REACH, side="left"))
        b = int(np.searchsorted(v[0], int(end) + PHASE_REACH, side="right"))
        if b <= a:
            return None
        return v[0][a:b], v[1][a:b], v[2][a:b], v[3][a:b]

    def rows(self, chrom: str, start: int, end: int):
        """The same as (pos, a1 letter, a2 letter, ps) tuples - haplotag's form."""
        v = self.of(chrom, start, end)
        if v is None:
            return []
        return [(p, _NT16[x], _NT16[y], s) for p, x, y, s in zip(v[0].tolist(), v[1].tolist(), v[2].tolist(), v[3].tolist())]

    @staticmethod
    def from_rows(rows) -> "Sites":
        """From (contig, pos, a1 letter, a2 letter, ps) rows in any order; a second row at a contig and position is dropped."""
        by = {}
        for c, p, x, y, s in rows:
            by.setdefault(c, {}).setdefault(int(p), (_NT16.index(x.upper()), _NT16.index(y.upper()), int(s)))
        out = {}
        for c, d in by.items():
            pos = sorted(d)
            out[c] = (np.asarray(pos, dtype=np.int64), np.asarray([d[p][0] for p in pos], dtype=np.uint8),
                      np.asarray([d[p][1] for p in pos], dtype=np.uint8), np.asarray([d[p][2] for p in pos], dtype=np.int64))
        return Sites(out)


_sites_cache: dict = {}


def read_sites(path: str, sample: Optional[str] = None, contigs=None) -> Sites:
    """The sites of a phased VCF (plain or gzip / bgzip compressed; read whole with the standard library, once per process, no
    index).  The sample is the first sample column or the one named.  With alleles = [REF] + ALT.split(','), a record is a site
    when REF is one letter, the sample's GT is `x|y` with integers x != y, and alleles[x] and alleles[y] are each one letter of
    ACGT in either case; a1 = alleles[x] is what haplotype 1 carries, a2 = alleles[y] haplotype 2.  ps = the integer value of
    the PS FORMAT key, 0 where it is absent or '.'.  FILTER is ignored.  Of the sites at one contig and position the first
    stands.  contigs: the names to keep (the BAM's), None for all.  ValueError for a VCF without a sample column or without
    the sample that was named."""
    import gzip
    import os
    st = os.stat(path)
    key = (os.path.abspath(path), sample, st.st_mtime_ns, st.st_size)
    rows = _sites_cache.get(key)
    if rows is None:
        with open(path, "rb") as f:
            raw = f.read()
        text = (gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw).decode("utf-8", "replace")
        rows = []
        col = None
        for ln in text.splitlines():
            if ln.startswith("##") or not ln.strip():
                continue
            f = ln.split("\t")
            if ln.startswith("#"):
                names = f[9:]
                if not names:
                    raise ValueError("%s has no sample column" % path)
                if sample is None:
                    col = 9
                elif sample in names:
                    col = 9 + names.index(sample)
                else:
                    raise ValueError("%s has no sample %r (it has: %s)" % (path, sample, ", ".join(names)))
                continue
            if col is None:
                raise ValueError("%s has no #CHROM header line" % path)
            if len(f) <= col or len(f[3]) != 1:
                continue
            keys = f[8].split(":")
            vals = f[col].split(":")
            if "GT" not in keys or keys.index("GT") >= len(vals):
                continue
            gt = vals[keys.index("GT")].split("|")
            if len(gt) != 2 or not (gt[0].isdigit() and gt[1].isdigit()) or int(gt[0]) == int(gt[1]):
                continue
            alleles = [f[3]] + f[4].split(",")
            x, y = int(gt[0]), int(gt[1])
            if x >= len(alleles) or y >= len(alleles):
                continue
            a1, a2 = alleles[x].upper(), alleles[y].upper()
            if len(a1) != 1 or len(a2) != 1 or a1 not in "ACGT" or a2 not in "ACGT":
                continue
            ps = 0
            if "PS" in keys and keys.index("PS") < len(vals):
                try:
                    ps = int(vals[keys.index("PS")])
                except ValueError:
                    ps = 0
            rows.append((f[0], int(f[1]), a1, a2, ps))
        if col is None:
            raise ValueError("%s has no #CHROM header line" % path)
        if len(_sites_cache) > 8:
            _sites_cache.clear()
        _sites_cache[key] = rows
    return Sites.from_rows(r for r in rows if contigs is None or r[0] in contigs)


def cigar_ops(cigar):
    """A CIGAR as (length, operation letter) pairs: from SAM text, from BAM's packed uint32 operations, or from such pairs."""
    global _CIGAR_TEXT
    if isinstance(cigar, str):
        if _CIGAR_TEXT is None:
            import re
            _CIGAR_TEXT = re.compile(r"(\d+)([MIDNSHP=X])")
        return [(int(n), op) for n, op in _CIGAR_TEXT.findall(cigar)]
    if isinstance(cigar, np.ndarray):
        return [(c >> 4, _CIGAR_OPS[c & 15] if (c & 15) < 9 else "?") for c in cigar.tolist()]
    return list(cigar)


def haplotag(pos: int, cigar, seq: str, sites):
    """(hap, ps) of an alignment record from the phased sites of its locus - (pos, a1, a2, ps) tuples in position order, no
    position twice.  pos: the record's 1-based POS; cigar: its operations (cigar_ops' forms; the CG:B,I array where the record
    has the long-CIGAR form); seq: its SEQ.  The walk keeps SAM's cursors (not cigar2alignstart_by_pos's): M = X advance the
    reference and the query cursor, I S the query cursor, D N the reference cursor, H P neither.  A site at reference position
    v inside an M, = or X operation that covers [rr, rr + n) with query cursor q reads the base SEQ[q + v - rr]: a1 is one vote
    for haplotype 1 in the site's phase set, a2 one for haplotype 2, anything else (N, =, another letter, a site inside D / N
    or outside the alignment) none.  Among the phase sets with a vote the one with the most votes n1 + n2 is taken, ties to the
    numerically smallest; hap = 1 when its n1 > n2, 2 when n2 > n1; on n1 == n2 or without a vote (0, None)."""
    sites = sites if isinstance(sites, list) else list(sites)
    ns = len(sites)
    if ns == 0:
        return 0, None
    votes = {}
    rr, q, si = int(pos), 0, 0
    for n, op in cigar_ops(cigar):
        if op in "M=X":
            while si < ns and sites[si][0] < rr:
                si += 1
            while si < ns and sites[si][0] < rr + n:
                v, a1, a2, ps = sites[si]
                qi = q + v - rr
                b = seq[qi].upper() if qi < len(seq) else ""
                if b == a1.upper() or b == a2.upper():
                    t = votes.setdefault(int(ps), [0, 0])
                    t[0 if b == a1.upper() else 1] += 1
                si += 1
            rr += n
            q += n
        elif op in "IS":
            q += n
        elif op in "DN":
            rr += n
        if si >= ns:
            break
    if not votes:
        return 0, None
    ps = min(votes, key=lambda p: (-(votes[p][0] + votes[p][1]), p))
    n1, n2 = votes[ps]
    return (1, ps) if n1 > n2 else (2, ps) if n2 > n1 else (0, None)


def device_site_tables(sites: Optional[Sites], chroms, starts, ends):
    """The sites of many regions as vapor_bam_chop_device_haplotag takes them: site_first (int32, n + 1), the regions' slices
    as 8-byte entries (int32 pos, uint8 a1, a2, the phase set's index in the region's own table, 0), ps_first (int32, n + 1)
    and the regions' tables of phase-set values (int64, ascending).  A region with more than PHASE_SETS_DEVICE distinct phase
    sets gets an empty slice and a table of PHASE_SETS_DEVICE + 1 entries: the library leaves such a region to the host route."""
    n = len(chroms)
    site_first, ps_first = np.zeros(n + 1, dtype=np.int32), np.zeros(n + 1, dtype=np.int32)
    ent, tabs = [], []
    dt = np.dtype([("pos", "<i4"), ("a1", "u1"), ("a2", "u1"), ("idx", "u1"), ("pad", "u1")])
    ns = nt = 0
    for g in range(n):
        v = sites.of(chroms[g], int(starts[g]), int(ends[g])) if sites is not None else None
        if v is not None and int(v[0][-1]) >= 1 << 31:      # (a BAM position is 32-bit: no record reaches such a site)
            v = tuple(x[v[0] < (1 << 31)] for x in v)
            v = v if len(v[0]) else None
        if v is not None:
            tab, idx = np.unique(v[3], return_inverse=True)
            if len(tab) > PHASE_SETS_DEVICE:
                tabs.append(tab[:PHASE_SETS_DEVICE + 1])
                nt += PHASE_SETS_DEVICE + 1
            else:
                e = np.zeros(len(v[0]), dtype=dt)
                e["pos"], e["a1"], e["a2"], e["idx"] = v[0], v[1], v[2], idx
                ent.append(e)
                tabs.append(tab)
                ns += len(e)
                nt += len(tab)
        site_first[g + 1], ps_first[g + 1] = ns, nt
    return (site_first, np.concatenate(ent) if ent else np.zeros(0, dtype=dt), ps_first,
            np.concatenate(tabs).astype(np.int64) if tabs else np.zeros(0, dtype=np.int64))


# ---------------------------------------------------------------------------------------------
# the groups of a locus
# ---------------------------------------------------------------------------------------------
def phase_set(x):
    """(tagged, P) of the kept records x ([read, miss_bp, qname, hap, ps] each): P = the ps value most frequent among the
    records with hap != 0, ties to the numerically smallest value, None ("none") below every number; tagged = False when no
    record has hap != 0 (P is None then)."""
    count = {}
    for r in x:
        if r[3]:
            count[r[4]] = count.get(r[4], 0) + 1
    if not count:
        return False, None
    top = max(count.values())
    best = [v for v, c in count.items() if c == top]
    return True, (None if None in best else min(best))


class PhasedReads(list):
    """Group A's read list (today's list: minimize_pacbio_read_list of every kept record) with the selection beside it:
    `tagged` / `ps` (phase_set), `groups` = the read lists of A, H1 and H2, `union` = the distinct records of the three lists in
    record order, `mask[u]` = membership of union[u] (bit 0 A, bit 1 H1, bit 2 H2), `pos[g][t]` = index into union of read t of
    group g."""
    tagged, ps, groups, union, mask, pos = False, None, (), (), (), ()


def select(x, ideal_list_length: int = 20) -> PhasedReads:
    """The three groups of a phased locus from its kept records x (before the cap of 20; file order):  A = all of x, Hh = the
    records with hap == h and ps == P; each group's list is minimize_pacbio_read_list (SF:1091-1102) of the group."""
    from .seqio import minimize_pacbio_read_list
    tagged, ps = phase_set(x)
    groups = [minimize_pacbio_read_list(list(x), ideal_list_length)]
    for h in (1, 2):
        groups.append(minimize_pacbio_read_list([r for r in x if tagged and r[3] == h and r[4] == ps], ideal_list_length))
    out = PhasedReads(groups[0])
    mask = {}
    for g, lst in enumerate(groups):
        for r in lst:
            mask[id(r)] = mask.get(id(r), 0) | (1 << g)
    union, at = [], {}
    for r in x:
        if id(r) in mask:
            at[id(r)] = len(union)
            union.append(r)
    out.tagged, out.ps, out.groups, out.union = tagged, ps, tuple(groups), union
    out.mask = [mask[id(r)] for r in union]
    out.pos = tuple([at[id(r)] for r in lst] for lst in groups)
    return out


def member_words(sel: PhasedReads) -> List[int]:
    """The selection as one word per read of the union, the way vapor_bam_chop_device_tagged hands it over: bits 0-2 the
    read is in the list of A / H1 / H2, bits 8-15, 16-23, 24-31 its position in that list."""
    w = list(sel.mask)
    for g in range(3):
        for t, u in enumerate(sel.pos[g]):
            w[u] |= t << (8 + 8 * g)
    return w


def select_numbers(miss, hap, ps, max_keep: int = 20):
    """select() over a region's kept records given as numbers (ps: PS_NONE for none): (tagged, P or PS_NONE, indices of the
    union's records, their member words) - the host form of the device's answer (vapor_bam_chop_device_tagged)."""
    x = [[i, m, None, h, (None if p == PS_NONE else p)] for i, (m, h, p) in enumerate(zip(miss.tolist(), hap.tolist(), ps.tolist()))]
    sel = select(x, max_keep)
    return sel.tagged, (PS_NONE if sel.ps is None else sel.ps), [r[0] for r in sel.union], member_words(sel)


def split_scores(member, scores, num_reads_cff: int):
    """A region's per-read scores (one per read of its union, NaN for a skipped read) split by the member words: the score
    lists of A, H1 and H2 in list order, skipped reads left out; None for H1 / H2 when the group's list has no more than
    num_reads_cff reads."""
    out = []
    for g in range(3):
        idx = [u for u in range(len(member)) if (member[u] >> g) & 1]
        idx.sort(key=lambda u: (member[u] >> (8 + 8 * g)) & 255)
        if g and not len(idx) > num_reads_cff:
            out.append(None)
        else:
            out.append([scores[u] for u in idx if scores[u] == scores[u]])
    return out


# ---------------------------------------------------------------------------------------------
# what the scores of a phased locus carry, and the columns
# ---------------------------------------------------------------------------------------------
class Phased(list):
    """A phased locus's score list (group A's, as without the option) with `phase` = (tagged, P, H1, H2): Hh = the scores of
    group h's reads (the skipped ones left out, as in the main list), or None for a group that is not reported (its list has
    no more than num_reads_cff reads)."""
    phase = None


def pack(phase) -> List[float]:
    """`phase` as floats, for the gather across ranks: [tagged, P is a number, P, reported1, n1, scores1 .., reported2, n2,
    scores2 ..] (a phase set - at most 2^32 - 1 - list lengths and scores are float64 exactly); [] for a locus that is not phased."""
    if phase is None:
        return []
    tagged, ps, h1, h2 = phase
    out = [float(bool(tagged)), float(ps is not None), float(ps or 0)]
    for h in (h1, h2):
        out += [float(h is not None), float(len(h or ()))] + [float(s) for s in (h or ())]
    return out


def unpack(v):
    if v is None or len(v) == 0:
        return None
    tagged, has, ps = bool(v[0]), bool(v[1]), int(v[2])
    hs, p = [], 3
    for _ in range(2):
        rep, n = bool(v[p]), int(v[p + 1])
        hs.append([float(s) for s in v[p + 2:p + 2 + n]] if rep else None)
        p += 2 + n
    return tagged, (ps if has else None), hs[0], hs[1]


def counts(scores):
    """(k, l) of a group's scores: the scored reads, and those whose score is non-positive under finish.rounded_nonpositive."""
    from .finish import rounded_nonpositive
    s = np.asarray(scores, dtype=np.float64)
    return int(s.size), int(rounded_nonpositive(s).sum())


def allele(k: int, l: int) -> str:
    """'1' when more of the k scored reads are positive than not, '0' when fewer, '.' on a tie or without a scored read."""
    if k - l > l:
        return "1"
    if k - l < l:
        return "0"
    return "."


def quality(k: int, l: int):
    """The reference's 5 % error model (log_likelihood_calcu, SF:2071-2077) restricted to the two haploid genotypes: the log10
    likelihood ratio of the called allele against the other."""
    return abs(k - 2 * l) * (np.log(0.95 / 0.05) / np.log(10))


def genotype(kl1, kl2):
    """(VaPoR_PGT, VaPoR_PGQ) from (k, l) of H1 and of H2, None for a group that is not reported."""
    a = [allele(*kl) if kl is not None else "." for kl in (kl1, kl2)]
    if a == [".", "."]:
        return ".", "."
    if "." in a:
        return "|".join(a), "."
    return "|".join(a), str(min(quality(*kl1), quality(*kl2)))


def columns(phase, tails=None) -> List[str]:
    """The nine extra fields of a row (COLUMNS); nine '.' for a locus that is not phased.  A reported group's QS, GS and Rec are
    finish.row_tail's of its scores, written as the main columns are (tails: those of H1 and H2 where the caller has them)."""
    from .finish import row_tail
    if phase is None:
        return ["."] * 9
    tagged, ps, h1, h2 = phase
    out = [str(ps) if tagged and ps is not None else "."]
    out += list(genotype(*[counts(h) if h is not None else None for h in (h1, h2)]))
    for q, h in enumerate((h1, h2)):
        if h is None:
            out += [".", ".", "."]
        else:
            t = tails[q] if tails is not None else row_tail(h)
            out += [str(t[0]), str(t[1]), str(t[4])]
    return out


def columns_many(phases) -> List[List[str]]:
    """columns() for every row of a table, the groups' row tails through finish.row_tails (one call of the library's host helper
    for the whole table, as the main columns are made)."""
    from .finish import row_tails
    tails = row_tails([h if h is not None else [] for ph in phases for h in ((ph[2], ph[3]) if ph is not None else ([], []))])
    return [columns(ph, tails[2 * t:2 * t + 2]) for t, ph in enumerate(phases)]

"""Haplotype-resolved validation (`vapor bed | vcf --phased`; not in the reference: DESIGN.md §4.13).

A haplotagged BAM carries `HP:i:1|2` and a phase set `PS:i:n` on its alignments.  This module holds the one statement of what
those tags mean here - the tag rule (`tags_from_aux`, `tags_from_sam`), the groups of a locus (`select`), the phased genotype
(`allele`, `quality`) and the nine columns (`columns`) - for the three readers (bamio's Python reader, the library's
vapor_bam_chop_tagged, SAM text), the drivers and the writer.
"""
from __future__ import annotations

import struct
from typing import List, Optional

import numpy as np

COLUMNS = ("VaPoR_PS", "VaPoR_PGT", "VaPoR_PGQ", "VaPoR_H1_QS", "VaPoR_H1_GS", "VaPoR_H1_Rec", "VaPoR_H2_QS", "VaPoR_H2_GS",
           "VaPoR_H2_Rec")
PS_NONE = -(1 << 63)          # "no PS field" where a phase set travels as an int64 (vapor_bam_chop_tagged's meta)

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

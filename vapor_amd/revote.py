"""`vapor bed | vcf --realign --realign-polish --realign-revote`: every read of a locus aligned once more, against
the polished allele, and the seven vote columns given a second time from d_ref - d_pol, with the edits the polish bought.  This
module is the rule - exact integers: `spell` (the polished allele as plane codes, and where every column's own symbol stands in
it), `statement` (the Python statement the three kernels of vapor_revote.h are held to, built on realign.statement), `eight` (the
columns and their gate) - and the mode's surface for cli.py and the VCF writer: `over(src)` wraps the source the columns follow
(polish, or junction where `--realign-junction` is given too) with INFO, COLUMNS, pack, unpack and columns_many.  The device spells
and aligns (Engine.realign_revote; pipeline.realign_requests makes the call in place of the polish's); there is no other route."""
from __future__ import annotations

from typing import List

import numpy as np

from . import polish, realign

E_ARG = -4                     # VAPOR_E_ARG (_lib.E_ARG)

INFO = (
    ("VaPoR_RA2_ALT", "Integer", "1", "Reads that align better to the polished alt allele than to the reference allele, by at least 10 edits (--realign-revote)"),
    ("VaPoR_RA2_REF", "Integer", "1", "Reads that align better to the reference allele than to the polished alt allele, by at least 10 edits (--realign-revote)"),
    ("VaPoR_RA2_NC", "Integer", "1", "Reads whose alignments to the reference and to the polished alt allele differ by fewer than 10 edits (--realign-revote)"),
    ("VaPoR_RA2_VAF", "Float", "1", "Allele fraction of the second vote, VaPoR_RA2_ALT / (VaPoR_RA2_ALT + VaPoR_RA2_REF) (--realign-revote)"),
    ("VaPoR_RA2_GT", "String", "1", "Genotype of the second vote, by VaPoR_RA_GT's rule (--realign-revote)"),
    ("VaPoR_RA2_GQ", "Integer", "1", "Quality of VaPoR_RA2_GT, by VaPoR_RA_GQ's rule (--realign-revote)"),
    ("VaPoR_RA2_Rec", "Integer", ".", "Per read, its edit distance to the reference allele minus that to the polished alt allele (--realign-revote)"),
    ("VaPoR_RA2_GAIN", "Integer", "1", "Edits the piled reads lose on the polished alt allele, summed: d_alt - d_pol (--realign-revote)"),
)
COLUMNS = tuple(i[0] for i in INFO)

_TEXT_OF_CODE = "ACGTacgtNn?????*"   # a symbol that realign.statement reads as the plane code does: 8, 9 and 15 match nothing


def codes_of(seq, upper: bool = False) -> np.ndarray:
    """The plane codes of a sequence: A C G T 0..3, a c g t 4..7, N and the IUPAC letters 8, their lower case 9, every other byte
    15; with `upper` (a VAPOR_SEQ_UPPER twin) a lower-case letter takes its upper-case letter's code."""
    table = np.full(256, 15, dtype=np.uint8)
    for v, ch in enumerate("ACGT"):
        table[ord(ch)] = v
        table[ord(ch.lower())] = v if upper else v + 4
    for ch in "NRYSWKMBDHV":
        table[ord(ch)] = 8
        table[ord(ch.lower())] = 8 if upper else 9
    raw = seq.encode("latin-1") if isinstance(seq, str) else bytes(seq)
    return table[np.frombuffer(raw, dtype=np.uint8)]


def text_of(codes) -> str:
    """A text whose plane codes are `codes` (0..9 and 15)."""
    return "".join(_TEXT_OF_CODE[int(c)] for c in codes)


def spell(codes, calls, sites, ins):
    """(spelt, own) of a locus: the codes a[0 .. len) of its alt allele under 4.25's calls, sites and inserted text.  The flagged
    columns (call bit 3) are numbered k = 0, 1, .. in column order; for q ascending a flagged column emits the sites[k][1] bases
    of ins[k] first, as codes 0..3, then the column's own symbol: KEEP a[q] unchanged, a call 0..3 that code, DELETE nothing.
    own (len + 1 int32): own[q] = the symbols emitted before column q's own symbol, its site's text included; own[len] = plen."""
    out, own, k = [], [], 0
    for q, a in enumerate(codes):
        call = int(calls[q])
        if call & polish.SITE_BIT:
            out += ["ACGT".index(chr(int(v))) for v in ins[k][:int(sites[k][1])]]
            k += 1
        own.append(len(out))
        call &= 7
        if call == polish.KEEP:
            out.append(int(a))
        elif call < 4:
            out.append(call)
    own.append(len(out))
    return np.asarray(out, dtype=np.uint8), np.asarray(own, dtype=np.int32)


def statement(votes, allele, calls, sites, ins, band: int, upper: bool = False, max_len: int = 65535):
    """(lout, vout, spelt, own) of a locus whose polish came back with status 0: `votes` its vote pairs [(read, off2)], off2 in
    the columns of `allele`.  lout {vstatus, plen, 0, 0}, vstatus E_ARG for plen > max_len (VAPOR_MAX_SEQ_LEN); vout a row a vote
    pair {d_pol, 0, off2', m'} with off2' = own[off2], m' = plen - off2' and d_pol = realign.statement of the read against the
    polished symbols from off2' on, or {-1, E_ARG, 0, 0} for an off2 outside 0 .. len and {-1, vstatus, 0, 0} where vstatus is
    not 0."""
    spelt, own = spell(codes_of(allele, upper), calls, sites, ins)
    plen = len(spelt)
    vstatus = E_ARG if plen > max_len else 0
    text = text_of(spelt) if not vstatus else ""
    vout = np.zeros((len(votes), 4), dtype=np.int32)
    for t, (read, off2) in enumerate(votes):
        off2 = int(off2)
        if vstatus or not 0 <= off2 <= len(allele):
            vout[t] = (-1, vstatus or E_ARG, 0, 0)
            continue
        at = int(own[off2])
        vout[t] = (realign.statement(read, text, at, band), 0, at, plen - at)
    return np.asarray([vstatus, plen, 0, 0], dtype=np.int32), vout, spelt, own


class Revote:
    """What `--realign-revote` knows of a locus: the status of its second vote (the locus's re-vote status, else the first status
    a vote pair came back with; 0 where all is well) and per read, in read order, d_ref of the first call and d_pol.  Rides on the
    locus's realign.Payload as `.revote`; travels in the gather."""
    __slots__ = ("status", "d_ref", "d_pol")

    def __init__(self, status, d_ref, d_pol):
        self.status = int(status)
        self.d_ref, self.d_pol = tuple(int(v) for v in d_ref), tuple(int(v) for v in d_pol)
        if len(self.d_ref) != len(self.d_pol):
            raise ValueError("revote: one d_ref and one d_pol a read")


def applies(p) -> bool:
    """The gate: the locus has a payload, its polish status is 0, at least MIN_COV reads were piled, its re-vote status is 0 and
    every vote pair came back with status 0 (a Revote of status 0 with a d_pol for every read)."""
    if p is None or p.polish is None or p.revote is None:
        return False
    return (p.polish.stats[polish.STATUS] == 0 and p.polish.stats[polish.PAIRS] >= polish.MIN_COV and p.revote.status == 0 and
            len(p.revote.d_pol) == len(p))


def eight(p) -> List[str]:
    """The eight columns: realign's seven of diff2 = d_ref - d_pol, then GAIN = the sum over the piled reads - those whose first
    diff is at least MARGIN - of d_alt - d_pol; '.' where the gate does not hold."""
    if not applies(p):
        return ["."] * 8
    rv = p.revote
    diff2 = realign.votes(rv.d_ref, rv.d_pol)
    gain = sum(d2 - d for d, d2 in zip(p, diff2) if d >= realign.MARGIN)      # d_alt - d_pol = (d_ref - d_pol) - (d_ref - d_alt)
    return realign.columns(realign.Payload(diff2)) + [str(gain)]


def _read(flat, at):
    """A Revote from its floats {status, n, d_pol x n, d_ref x n} at `at`, and where they end."""
    n = int(flat[at + 1])
    return Revote(flat[at], flat[at + 2 + n:at + 2 + 2 * n], flat[at + 2:at + 2 + n]), at + 2 + 2 * n


SECTION = realign.Section("revote", INFO, eight, lambda rv: (rv.status, len(rv.d_pol)) + rv.d_pol + rv.d_ref, _read)


def over(src) -> realign.Chain:
    """The surface of a run with `--realign-revote`: the sections of the source the columns follow - polish, or junction -, then
    this one."""
    return realign.Chain(src.SECTIONS + (SECTION,))


# (the run without `--realign-junction`: polish's columns, then the eight)
_PLAIN = over(polish)
columns, pack, unpack, columns_many = _PLAIN.columns, _PLAIN.pack, _PLAIN.unpack, _PLAIN.columns_many

"""Locus drivers: allele-string construction, read selection and scorer choice per SV type
(component #2; reference SF:1490-1933).

Each driver is a generator.  It does its host-side string work itself and *yields* the two
kinds of device work the reference does inline -

    Window(seq)                             -> window_size_refine(seq)            (SF:2030-2046)
    Score(kind, ref_seq, alt_seq, reads, k) -> per read x the drivers' own reduction of
                                               calcu_vapor_single_read_score_*(ref, alt, x, k): the score
                                               1 - b/a, or None where the reference skips the read
                                               (`0 in [a, b]`, e.g. SF:1913); 'del' takes the smaller of the
                                               abs_dis and within_10Perc scores (SF:1718-1726)

- and receives the results back through send().  Run one generator at a time
(`pipeline.run_sync`) and it behaves like the reference's function of the same name; run many
in lockstep (`pipeline.run_batch`) and the pending requests of all loci go to the GPU as one
batch.  The control flow, fallbacks and quirks of the reference are kept, including the places
where it raises (cited inline).
"""
from __future__ import annotations

from typing import List

from . import realign, seqio

default_flank_length = 500       # SF:21-22
default_max_sv_test = 10000      # SF:25-26


class Window:
    __slots__ = ("seq",)

    def __init__(self, seq: str):
        self.seq = seq


class Score:
    """kind: 's1' abs_dis_m1b, 's2' within_10Perc_m1b, 's3' directed_dis_m1b_redefine_diagnal,
    'del' = s1 and s2 for the same reads.  Result: one score (float) or None per read."""
    __slots__ = ("kind", "ref_seq", "alt_seq", "reads", "k")

    def __init__(self, kind, ref_seq, alt_seq, reads, k):
        self.kind, self.ref_seq, self.alt_seq, self.reads, self.k = kind, ref_seq, alt_seq, reads, k


class ScoreGrid:
    """Breakpoint refinement (vapor_refine): one window, one set of reads, `alts` = the candidate alleles (each a _cat of
    slices of `ref_seq`; the first is the call itself), all scored as Score(kind, ref_seq, alt, reads, k) would be.  Result: a
    refine.GridResult - the winner among the candidates (refine.pick), its per-read scores, its record and candidate 0's."""
    __slots__ = ("kind", "ref_seq", "alts", "reads", "k")

    def __init__(self, kind, ref_seq, alts, reads, k):
        self.kind, self.ref_seq, self.alts, self.reads, self.k = kind, ref_seq, list(alts), reads, k


class Figure:
    """make_event_figure_1 (SF:1072-1089) request; executors may render it or drop it."""
    __slots__ = ("scores", "best_read", "k", "ref_seq", "alt_seq", "name")

    def __init__(self, scores, best_read, k, ref_seq, alt_seq, name):
        self.scores, self.best_read, self.k = scores, best_read, k
        self.ref_seq, self.alt_seq, self.name = ref_seq, alt_seq, name


def _collect(results, reads, scores: List[float], keep=None):
    """The per-read loop every driver repeats (e.g. SF:1909-1915): a read counts when neither scorer output is 0
    (`keep`: a flag per read, for the reads that were handed to the executor at all; the executor
    hands such a read over as None, the others as 1 - b/a; the scorers never produce NaN, so
    vapor_dup_inv_VapoR's extra isnan test, SF:1629, changes nothing); returns the read with the best score so
    far (ties: the later read)."""
    best = ""
    it = iter(results)
    top = max(scores) if scores else None
    for t, x in enumerate(reads):
        if keep is not None and not keep[t]:
            continue
        s = next(it)
        if s is None:
            continue
        scores.append(s)
        if top is None or s >= top:          # (`scores[-1] == max(scores)` of the reference, without the scan)
            top = s
            best = x
    return best


def _scores(phased):
    """A driver's score list: a plain list, or with `--phased` a phase.Phased (a list that can carry the groups' scores)."""
    if not phased:
        return []
    from .phase import Phased
    return Phased()


def _score_phased(kind, ref_seq, alt_seq, reads, k, scores, num_reads_cff, keep_fn=None):
    """The Score request and the per-read loop of a simple driver for a phased locus (`--phased`; not in the
    reference).  `reads` is a phase.PhasedReads: group A's list - today's list - with the lists of H1 and H2 beside it.  The
    distinct reads of the three lists go into ONE Score request (every read is scored once); group A's part of the answer
    goes through _collect exactly as the unphased driver's answer does, and the parts of H1 and H2 ride on `scores.phase`
    for the writer.  keep_fn: the INS driver's per-read N rule (SF:1878), applied to every read of the union.  A group whose
    list has no more than num_reads_cff reads - the gate group A has passed - is not reported (None)."""
    union = reads.union
    kept = [keep_fn(x) for x in union] if keep_fn is not None else [True] * len(union)
    used = [x for x, f in zip(union, kept) if f]
    res = (yield Score(kind, ref_seq, alt_seq, used, k)) if used else []
    it = iter(res)
    got = [next(it) if f else None for f in kept]            # per read of the union: its score, None where it was skipped
    pos_a = reads.pos[0]
    best = _collect([got[u] for u in pos_a if kept[u]], reads, scores, keep=[kept[u] for u in pos_a])
    halves = []
    for g in (1, 2):
        if len(reads.groups[g]) > num_reads_cff:
            halves.append([got[u] for u in reads.pos[g] if got[u] is not None])
        else:
            halves.append(None)
    scores.phase = (reads.tagged, reads.ps, halves[0], halves[1])
    return best


def _window(seq):
    res = yield Window(seq)
    return res[0]


def _rc(seq: str) -> str:
    return seqio.reverse(seqio.complementary(seq))


class Allele(str):
    """An allele string that remembers how the driver built it: `segs` = [(parent string, off, len, revcomp), ...] - slices of
    windows the driver has read (and of an insertion's sequence), in order.  It IS the string (every consumer that wants
    text - figures, the window check, the reference-named functions - sees a str); the executors hand the segments to the
    library instead of the bytes (include/vapor_hip.h, vapor_seqset_create_derived): the device assembles the allele from
    the window it already has, and a read is joined once against the window and the alleles derived from it.
    `segs` is None when the text is not a concatenation of slices (complementary() drops characters outside ATGCN / atgcn,
    SF:471-478: a reversed slice that lost one is uploaded as bytes)."""
    segs = None


def _cat(*parts) -> Allele:
    """''.join of the parts, each (s, a, b) = s[a:b] or (s, a, b, True) = reverse(complementary(s[a:b])) with Python's slice
    rules (negative and None bounds), as an Allele that knows its segments."""
    text, segs = [], []
    for part in parts:
        src, a, b = part[0], part[1], part[2]
        i0, i1, _ = slice(a, b).indices(len(src))
        n = max(0, i1 - i0)
        piece = src[i0:i1]
        rc = len(part) > 3 and part[3]
        if rc:
            piece = _rc(piece)
            if len(piece) != n:
                segs = None                 # complementary() dropped something: not a slice of anything any more
        text.append(piece)
        if segs is not None and n:
            base = getattr(src, "segs", None)
            if base is not None and not rc and len(base) == 1 and not base[0][3]:
                seg = (base[0][0], base[0][1] + i0, n, False)             # (a slice of a one-slice allele: of its parent)
            elif type(src) is str:
                seg = (src, i0, n, rc)
            else:
                segs = None
                continue
            last = segs[-1] if segs else None
            if last is not None and not seg[3] and not last[3] and last[0] is seg[0] and last[1] + last[2] == seg[1]:
                segs[-1] = (last[0], last[1], last[2] + n, False)         # (two forward slices that lie end to end: one slice)
            else:
                segs.append(seg)
    out = Allele("".join(text))
    out.segs = segs
    return out


def _within(window: str, w0: int, piece: str, a: int):
    """The _cat part for `piece` = the reference from coordinate `a` on, given a window that starts at coordinate `w0`: a
    slice of the window where the window really holds those bases (the usual case: the drivers fetch a block's bases again
    although they lie inside the window they already hold, e.g. SF:1809-1813), else the piece as text of its own."""
    off = a - w0
    if off >= 0 and len(piece) and window[off:off + len(piece)] == piece:
        return (window, off, off + len(piece))
    return (piece, None, None)


def _rcpart(part):
    return (part[0], part[1], part[2], True)


# ------------------------------------------------------------------------------------------
def vapor_simple_del(num_reads_cff, plt_li, bam_in, ref, sv_info, out_figure_name, phased=False):
    """vapor_simple_del_Vapor, SF:1701-1745.  phased (`--phased`, here and in the three drivers below): the reads come as a
    phase.PhasedReads and the Score request goes through _score_phased; nothing else differs."""
    flank = seqio.flank_length_calculate(sv_info)
    scores: List[float] = _scores(phased)
    ph = (True,) if phased else ()
    if sv_info[2] - sv_info[1] < default_max_sv_test:
        reads = seqio.simple_del_chop_pacbio_read_simple_short(bam_in, sv_info, flank, *ph)
        if len(reads) > num_reads_cff:
            ref_seq = seqio.ref_seq_readin(ref, sv_info[0], sv_info[1] - flank, sv_info[2] + flank)
            k = yield from _window(ref_seq)
            if not k == "Error":
                alt_seq = _cat((ref_seq, None, flank), (ref_seq, -flank, None))      # ref_seq[:flank] + ref_seq[-flank:], SF:1712
                if phased:
                    best = yield from _score_phased("del", ref_seq, alt_seq, reads, k, scores, num_reads_cff)
                else:
                    res = yield Score("del", ref_seq, alt_seq, reads, k)     # min of the two scorers' scores, SF:1718-1726
                    best = _collect(res, reads, scores)
                yield Figure(scores, best, k, ref_seq, alt_seq, out_figure_name)
    else:
        reads = seqio.simple_del_chop_pacbio_read_simple_short(bam_in, sv_info, flank, *ph)
        if len(reads) > num_reads_cff:
            ref_seq = seqio.ref_seq_readin(ref, sv_info[0], sv_info[1] - flank, sv_info[1] + flank)
            k = yield from _window(ref_seq)
            if not k == "Error":
                left = seqio.ref_seq_readin(ref, sv_info[0], sv_info[1] - flank, sv_info[1])
                alt_seq = _cat(_within(ref_seq, sv_info[1] - flank, left, sv_info[1] - flank),
                               (seqio.ref_seq_readin(ref, sv_info[0], sv_info[2], sv_info[2] + flank), None, None))
                k = yield from _window(alt_seq)
                if not k == "Error":
                    if phased:
                        best = yield from _score_phased("s2", ref_seq, alt_seq, reads, k, scores, num_reads_cff)
                    else:
                        res = yield Score("s2", ref_seq, alt_seq, reads, k)
                        best = _collect(res, reads, scores)
                    yield Figure(scores, best, k, ref_seq, alt_seq, out_figure_name)
    return scores


def vapor_bnd(num_reads_cff, plt_li, bam_in, ref, bnd_info, out_figure_name):
    """A breakend junction (`vapor vcf --bnd`; not in the reference): the long-deletion branch of
    vapor_simple_del_Vapor (SF:1727-1745) for [A, p, q - 1], its right piece taken on contig B - forward from q - 1 ('3to5',
    as the branch starts at END) or the reverse complement of B up to q ('3to3') - with the breakend's inserted bases between
    the pieces.  bnd_info = [A, p, B, q, CT, inserted bases] (cli.bnd_view)."""
    a, p, b, q, ct, ins = bnd_info
    flank = default_flank_length
    scores: List[float] = []
    reads = seqio.simple_del_chop_pacbio_read_simple_short(bam_in, [a, p], flank)
    if len(reads) > num_reads_cff:
        ref_seq = seqio.ref_seq_readin(ref, a, p - flank, p + flank)
        k = yield from _window(ref_seq)
        if not k == "Error":
            left = seqio.ref_seq_readin(ref, a, p - flank, p)
            if ct == "3to5":
                right = (seqio.ref_seq_readin(ref, b, q - 1, q - 1 + flank), None, None)
            else:
                right = (seqio.ref_seq_readin(ref, b, q - flank, q), None, None, True)
            alt_seq = _cat(_within(ref_seq, p - flank, left, p - flank), (ins, None, None), right)
            k = yield from _window(alt_seq)
            if not k == "Error":
                res = yield Score("s2", ref_seq, alt_seq, reads, k)
                best = _collect(res, reads, scores)
                yield Figure(scores, best, k, ref_seq, alt_seq, out_figure_name)
    return scores


def vapor_simple_inv(num_reads_cff, plt_li, bam_in, ref, sv_info, out_figure_name, phased=False):
    """vapor_simple_inv_Vapor, SF:1895-1933."""
    flank = seqio.flank_length_calculate(sv_info)
    scores: List[float] = _scores(phased)
    ph = (True,) if phased else ()
    if sv_info[2] - sv_info[1] < default_max_sv_test:
        ref_seq = seqio.ref_seq_readin(ref, sv_info[0], sv_info[1] - flank, sv_info[2] + flank)
        k = yield from _window(ref_seq)
        if not k == "Error":
            # ref_seq[:flank] + reverse(complementary(ref_seq[flank:-flank])) + ref_seq[-flank:], SF:1907
            alt_seq = _cat((ref_seq, None, flank), (ref_seq, flank, -flank, True), (ref_seq, -flank, None))
            k = yield from _window(alt_seq)
            if not k == "Error":
                reads = seqio.simple_chop_pacbio_read_simple_short(bam_in, sv_info, flank, *ph)
                if len(reads) > num_reads_cff:
                    if phased:
                        best = yield from _score_phased("s1", ref_seq, alt_seq, reads, k, scores, num_reads_cff)
                    else:
                        res = yield Score("s1", ref_seq, alt_seq, reads, k)
                        best = _collect(res, reads, scores)
                    yield Figure(scores, best, k, ref_seq, alt_seq, out_figure_name)
                    return scores
    ref_seq = seqio.ref_seq_readin(ref, sv_info[0], sv_info[1] - flank, sv_info[1] + flank)
    k = yield from _window(ref_seq)
    if not k == "Error":
        alt_seq = _cat((ref_seq, None, flank), (seqio.ref_seq_readin(ref, sv_info[0], sv_info[2] - flank, sv_info[2], "TRUE"), None, None))
        k = yield from _window(alt_seq)
        if not k == "Error":
            reads = seqio.simple_del_chop_pacbio_read_simple_short(bam_in, sv_info, flank, *ph)
            if len(reads) > num_reads_cff:
                if phased:
                    best = yield from _score_phased("s2", ref_seq, alt_seq, reads, k, scores, num_reads_cff)
                else:
                    res = yield Score("s2", ref_seq, alt_seq, reads, k)
                    best = _collect(res, reads, scores)
                yield Figure(scores, best, k, ref_seq, alt_seq, out_figure_name)
    return scores


def vapor_simple_tandup(num_reads_cff, plt_li, bam_in, ref, sv_info, out_figure_name, phased=False):
    """vapor_simple_tandup_Vapor, SF:1747-1784."""
    flank = seqio.flank_length_calculate(sv_info)
    scores: List[float] = _scores(phased)
    ph = (True,) if phased else ()
    if sv_info[2] - sv_info[1] < default_max_sv_test:
        ref_seq = seqio.ref_seq_readin(ref, sv_info[0], sv_info[1] - flank, sv_info[2] + flank)
        k = yield from _window(ref_seq)
        if not k == "Error":
            # ref_seq[:flank] + mid + mid + ref_seq[-flank:] with mid = ref_seq[flank:-flank], SF:1755
            alt_seq = _cat((ref_seq, None, flank), (ref_seq, flank, -flank), (ref_seq, flank, -flank), (ref_seq, -flank, None))
            k = yield from _window(alt_seq)
            if not k == "Error":
                reads = seqio.simple_chop_pacbio_read_simple_short(
                    bam_in, sv_info[:2] + [sv_info[1] + 2 * (sv_info[2] - sv_info[1])], flank, *ph)
                if len(reads) > num_reads_cff:
                    if phased:
                        best = yield from _score_phased("s3", ref_seq, alt_seq, reads, k, scores, num_reads_cff)
                    else:
                        res = yield Score("s3", ref_seq, alt_seq, reads, k)
                        best = _collect(res, reads, scores)
                    yield Figure(scores, best, k, ref_seq, alt_seq, out_figure_name)
                    return scores
    ref_seq = seqio.ref_seq_readin(ref, sv_info[0], sv_info[2] - flank, sv_info[2] + flank)
    k = yield from _window(ref_seq)
    if not k == "Error":
        left = seqio.ref_seq_readin(ref, sv_info[0], sv_info[2] - flank, sv_info[2])
        alt_seq = _cat(_within(ref_seq, sv_info[2] - flank, left, sv_info[2] - flank),
                       (seqio.ref_seq_readin(ref, sv_info[0], sv_info[1], sv_info[1] + flank), None, None))
        k = yield from _window(alt_seq)
        if not k == "Error":
            reads = seqio.simple_del_chop_pacbio_read_simple_short(bam_in, [sv_info[0], sv_info[2]], flank, *ph)
            if len(reads) > num_reads_cff:
                if phased:
                    best = yield from _score_phased("s2", ref_seq, alt_seq, reads, k, scores, num_reads_cff)
                else:
                    res = yield Score("s2", ref_seq, alt_seq, reads, k)
                    best = _collect(res, reads, scores)
                yield Figure(scores, best, k, ref_seq, alt_seq, out_figure_name)
    return scores


# ------------------------------------------------------------------------------------------
# `--both-ends` (not in the reference): every junction scored from both of its sides
# ------------------------------------------------------------------------------------------

def _junction_view(num_reads_cff, bam_in, ref, form, info, flank, mirror):
    """One more view of a junction, scored the way the long branches score theirs: reads of the window anchor +- flank, the gate
    len(reads) > num_reads_cff, _window(ref), _window(alt), Score('s2').  Returns the per-read scores, or None for a view that
    was gated out or whose k was "Error".  form / info name the alleles by the existing long branches:
        'del' [c, s, e]                 anchor c:s, ref R(c, s-F, s+F), alt R(c, s-F, s) + R(c, e, e+F)      (SF:1727-1745)
        'inv' [c, s, e]                 anchor c:s, ref as above, alt ref[:F] + rc(R(c, e-F, e))              (SF:1917-1933)
        'bnd' [A, p, B, q, CT, ins]     vapor_bnd's, CT 3to5 or 3to3
    mirror: an R view - `info` holds coordinates of the reverse-complemented contigs, written as the NEGATIVE of the contig's
    own (x^ = L + 1 - x with L + 1 taken as 0: L cancels).  R^(c, a, b) = rc(R(c, -b, -a)) then, and the reads are the
    right-anchored ones of the window -anchor +- F, which come reverse complemented (seqio._chop_records)."""
    if mirror:
        def fetch(c, a, b):
            return _rc(seqio.ref_seq_readin(ref, c, -b, -a))
    else:
        def fetch(c, a, b):
            return seqio.ref_seq_readin(ref, c, a, b)
    c, x = info[0], info[1]
    if mirror:
        reads = seqio.simple_del_chop_pacbio_read_simple_short(bam_in, [c, -x], flank, right=True)
    else:
        reads = seqio.simple_del_chop_pacbio_read_simple_short(bam_in, [c, x], flank)
    if not len(reads) > num_reads_cff:
        return None
    ref_seq = fetch(c, x - flank, x + flank)
    k = yield from _window(ref_seq)
    if k == "Error":
        return None
    if form == "del":
        alt_seq = _cat(_within(ref_seq, x - flank, fetch(c, x - flank, x), x - flank), (fetch(c, info[2], info[2] + flank), None, None))
    elif form == "inv":
        alt_seq = _cat((ref_seq, None, flank), (fetch(c, info[2] - flank, info[2]), None, None, True))
    else:
        b, q, ct, ins = info[2], info[3], info[4], info[5]
        if ct == "3to5":
            right = (fetch(b, q - 1, q - 1 + flank), None, None)
        else:
            right = (fetch(b, q - flank, q), None, None, True)
        alt_seq = _cat(_within(ref_seq, x - flank, fetch(c, x - flank, x), x - flank), (ins, None, None), right)
    k = yield from _window(alt_seq)
    if k == "Error":
        return None
    res = yield Score("s2", ref_seq, alt_seq, reads, k)
    scores: List[float] = []
    if _dedup_on():
        # (`--dedup-qname` rule V: the key of every read that contributes a score, built where _collect drops the others)
        res = list(res)
        scores = KeyedScores()
        scores.keys = [_read_key(x) for x, s in zip(reads, res) if s is not None]
    _collect(res, reads, scores)
    return scores


class KeyedScores(list):
    """A view's per-read scores with `keys`: per score the name key of its read (`--dedup-qname`, DESIGN.md 4.18 rule V)."""
    keys = None


def _dedup_on() -> bool:
    return bool(getattr(seqio.get_backend(), "dedup_qname", False))


def _read_key(x) -> int:
    """The name key of a read entry [read, miss_bp, slot]: seqio.name_key of a QNAME, the slot itself where the device route put
    the key there (seqio.prefetch_views)."""
    s = x[2]
    return int(s) if not isinstance(s, str) else seqio.name_key(s)


def both_ends_views(svtype, info, flank=default_flank_length):
    """The extra views of a locus's junction branch, in table order: (name, form, info, mirror) each, for
    _junction_view.  svtype DEL / INV / TANDUP with info [c, s, e]; BND with info [A, p, B, q, CT, ins] (cli.bnd_view with
    both_ends: CT may be 5to5, whose FIRST view is the locus's primary one)."""
    if svtype == "DEL":
        c, s, e = info[:3]
        return [("R@e", "del", [c, -e, -s], True)]
    if svtype == "TANDUP":
        c, s, e = info[:3]
        return [("R@s", "del", [c, -s, -e], True)]
    if svtype == "INV":
        c, s, e = info[:3]
        return [("L@e", "bnd", [c, e, c, s, "3to3", ""], False), ("R@e", "inv", [c, -e, -s], True),
                ("R@s", "bnd", [c, -s, c, -e, "3to3", ""], True)]
    a, p, b, q, ct, ins = info
    if ct == "3to5":
        return [("R@B", "bnd", [b, -q, a, -p, "3to5", seqio.rc_read(ins)], True)]
    if ct == "3to3":
        return [("L@B", "bnd", [b, q, a, p, "3to3", seqio.rc_read(ins)], False)]
    return [("R@A", "bnd", [a, -p, b, -q, "3to3", seqio.rc_read(ins)], True), ("R@B", "bnd", [b, -q, a, -p, "3to3", ins], True)]


def both_ends_windows(svtype, info):
    """Every read window vapor_both_ends may ask for, as (chrom, start, end, flank, right) - the windows of the type's own driver
    (short branch and junction branch) and of the extra views - for one extraction call per chunk (seqio.prefetch_views)."""
    out = []
    if svtype == "BND":
        flank = default_flank_length
        if info[4] != "5to5":
            out.append((info[0], info[1] - flank, info[1] + flank, flank, False))
    else:
        c, s, e = info[:3]
        flank = seqio.flank_length_calculate(info)
        if svtype == "DEL":
            out.append((c, s - flank, s + flank, flank, False))
        elif svtype == "INV":
            out += [(c, s - flank, e + flank, flank, False), (c, s - flank, s + flank, flank, False)]
        else:
            out += [(c, s - flank, s + 2 * (e - s) + flank, flank, False), (c, e - flank, e + flank, flank, False)]
        if svtype == "DEL" and e - s < default_max_sv_test:
            return out
    for _name, _form, v, mirror in both_ends_views(svtype, info, flank):
        x = -v[1] if mirror else v[1]
        out.append((v[0], x - flank, x + flank, flank, bool(mirror)))
    return out


class BothEnds(list):
    """The score list of a locus under `--both-ends` - the primary view's, as without the option - with `views`: per scored or
    gated view of its junction branch, in table order and the primary first, its per-read scores or None (gated out, or k
    "Error"); None for a locus without junction branch.  `view_keys` (`--dedup-qname`, DESIGN.md 4.18 rule V; else None): per
    view the name keys of the reads behind its scores, None for a view without scores - the same list `views.keys` holds, which is
    how it travels with the views (bothends.pack)."""
    views = None
    view_keys = None


def vapor_both_ends(svtype, num_reads_cff, plt_li, bam_in, ref, info, out_figure_name):
    """`--both-ends` for a DEL, INV or TANDUP record [c, s, e] or a breakend view [A, p, B, q, CT, ins]: the type's own driver
    runs as it is - its requests, its figure, its scores: the row's own columns -, and when it took its junction branch
    (a DEL of 10 kb or more; an INV or TANDUP that did not score its short branch; every breakend) the extra views of that
    junction follow (both_ends_views), none of them drawn.  A 5to5 breakend has no view in the reference's read model: its
    primary view is its first right-anchored one."""
    out = BothEnds()
    seen = []
    if svtype == "BND" and info[4] == "5to5":
        views = both_ends_views("BND", info)
        got = yield from _junction_view(num_reads_cff, bam_in, ref, views[0][1], views[0][2], default_flank_length, True)
        out.extend(got or [])
        out.views = [got]
        for _name, form, vinfo, mirror in views[1:]:
            out.views.append((yield from _junction_view(num_reads_cff, bam_in, ref, form, vinfo, default_flank_length, mirror)))
        _keyed_views(out)
        return out
    if svtype == "BND":
        gen = vapor_bnd(num_reads_cff, plt_li, bam_in, ref, info, out_figure_name)
        flank = default_flank_length
    else:
        gen = {"DEL": vapor_simple_del, "INV": vapor_simple_inv, "TANDUP": vapor_simple_tandup}[svtype](
            num_reads_cff, plt_li, bam_in, ref, info, out_figure_name)
        flank = seqio.flank_length_calculate(info)
    # the type's own driver, its Score requests noted on the way through - and with `--dedup-qname` the keys of the reads behind
    # the scores of its junction branch, from the request and the answer that pass here (the driver itself stays as it is)
    dedup = _dedup_on()
    prim_keys: List[int] = []
    try:
        req = next(gen)
        while True:
            if isinstance(req, Score):
                seen.append(req.kind)
            ans = yield req
            if dedup and isinstance(req, Score) and req.kind == "s2":
                ans = list(ans)
                prim_keys += [_read_key(x) for x, s in zip(req.reads, ans) if s is not None]
            req = gen.send(ans)
    except StopIteration as fin:
        scores = fin.value
    out.extend(scores)
    if svtype == "DEL":
        junction = not info[2] - info[1] < default_max_sv_test
    elif svtype == "BND":
        junction = True
    else:
        junction = not [k for k in seen if k != "s2"]        # (the short branch did not score: the driver fell through, SF:1917, 1769)
    if junction:
        out.views = [list(scores) if "s2" in seen else None]
        if dedup and out.views[0] is not None:
            if len(prim_keys) != len(scores):
                raise AssertionError("--dedup-qname: %d keys for %d scores of the primary view" % (len(prim_keys), len(scores)))
            out.views[0] = KeyedScores(scores)
            out.views[0].keys = prim_keys
        for _name, form, vinfo, mirror in both_ends_views(svtype, info, flank):
            out.views.append((yield from _junction_view(num_reads_cff, bam_in, ref, form, vinfo, flank, mirror)))
        _keyed_views(out)
    return out


def _keyed_views(out) -> None:
    """With `--dedup-qname`: out.views becomes a bothends.Views that carries the views' keys, out.view_keys names the same list."""
    if not _dedup_on():
        return
    from .bothends import Views
    v = Views(out.views)
    v.keys = [None if x is None else list(x.keys) for x in out.views]
    out.views, out.view_keys = v, v.keys


_REFINE_BASE = {"DEL": vapor_simple_del, "INV": vapor_simple_inv, "TANDUP": vapor_simple_tandup}
_REFINE_KIND = {"DEL": "del", "INV": "s1", "TANDUP": "s3"}


def refine_allele(svtype, window, flank, margin, ds, de):
    """The alt allele of candidate (ds, de) on the widened window W = ref[s - M - F : e + M + F]: with L = W[:F + M + ds],
    R = W[-(F + M - de):] and mid what lies between, DEL L + R, INV L + rc(mid) + R, TANDUP L + mid + mid + R.  At M = 0 these
    are the alleles of vapor_simple_del / _inv / _tandup (SF:1712, 1907, 1755)."""
    lo, hi = flank + margin + ds, -(flank + margin - de)
    if svtype == "DEL":
        return _cat((window, None, lo), (window, hi, None))
    if svtype == "INV":
        return _cat((window, None, lo), (window, lo, hi, True), (window, hi, None))
    return _cat((window, None, lo), (window, lo, hi), (window, lo, hi), (window, hi, None))


def vapor_refine(svtype, num_reads_cff, plt_li, bam_in, ref, sv_info, out_figure_name, margin, step, cipos=None, ciend=None):
    """`--refine M[:T]` (not in the reference) for a DEL, INV or TANDUP record: the short branch of the type's
    driver for the widened record [c, s - M, e + M] with the flank of the called record - its window, its reads, its gates in
    its order - and, instead of one allele, the grid of candidate breakpoints (refine.candidates) as one ScoreGrid request.
    Returns the winner's scores as a refine.Refined (info = the winner's a and b, candidate 0's QS, GS and positive scores).  A locus the
    short branch would not score that way - a long record, a window check that fails, too few reads - is not refined: the
    type's own driver runs on the called record, exactly as without the option, and its plain list comes back."""
    from . import refine
    base = _REFINE_BASE[svtype]
    c, s, e = sv_info[0], sv_info[1], sv_info[2]
    flank = seqio.flank_length_calculate(sv_info)
    wide = [c, s - margin, e + margin]
    grid = None
    if e - s < default_max_sv_test and wide[2] - wide[1] < default_max_sv_test and wide[1] - flank >= 1:
        cands = refine.candidates(margin, step, s, e, cipos, ciend)

        def alts(window):
            return [refine_allele(svtype, window, flank, margin, ds, de) for ds, de in cands]
        if svtype == "DEL":
            reads = seqio.simple_del_chop_pacbio_read_simple_short(bam_in, wide, flank)
            if len(reads) > num_reads_cff:
                ref_seq = seqio.ref_seq_readin(ref, c, wide[1] - flank, wide[2] + flank)
                k = yield from _window(ref_seq)
                if not k == "Error":
                    grid = (ref_seq, alts(ref_seq), reads, k)
        else:
            ref_seq = seqio.ref_seq_readin(ref, c, wide[1] - flank, wide[2] + flank)
            k = yield from _window(ref_seq)
            if not k == "Error":
                cand_alts = alts(ref_seq)
                k = yield from _window(cand_alts[0])           # (one k per locus: the candidates' scores are comparable)
                if not k == "Error":
                    end = wide[2] if svtype == "INV" else wide[1] + 2 * (wide[2] - wide[1])
                    reads = seqio.simple_chop_pacbio_read_simple_short(bam_in, wide[:2] + [end], flank)
                    if len(reads) > num_reads_cff:
                        grid = (ref_seq, cand_alts, reads, k)
    if grid is None:
        return (yield from base(num_reads_cff, plt_li, bam_in, ref, sv_info, out_figure_name))
    ref_seq, cand_alts, reads, k = grid
    got = yield ScoreGrid(_REFINE_KIND[svtype], ref_seq, cand_alts, reads, k)
    scores = refine.Refined()
    best = _collect(got.scores, reads, scores)
    ds, de = cands[got.winner]
    scores.info = (float(s + ds), float(e + de), float(got.rec0[0]), float(got.rec0[1]), float(got.rec0[5]))
    yield Figure(scores, best, k, ref_seq, cand_alts[got.winner], out_figure_name)
    return scores


class Realign:
    """`--realign`: the reads of a Score request against its two alleles.  Result: a realign.Payload - per read
    its edit distance to ref_seq[miss_bp:] minus that to alt_seq[miss_bp:] - or None when a pair came back with a status.
    `options` (a realign.Options; nothing asked by default) says what else the payload is to carry, each on the attribute of the
    flag's name: `trace` (`--realign-out`) every read's alignment to the allele it fits, as `.traces`, with
    `name` the locus as the files spell it; `polish` (`--realign-polish`, 4.25) the consensus of the ALT voters on the alt
    allele; `junction` (`--realign-junction`, 4.26) the one jump of the polished allele beside that of the call's; `revote`
    (`--realign-revote`, 4.27) every read's distance to the polished allele.  The four flags read through the request."""
    __slots__ = ("ref_seq", "alt_seq", "reads", "name", "options")

    def __init__(self, ref_seq, alt_seq, reads, name=None, options=realign.Options()):
        self.ref_seq, self.alt_seq, self.reads, self.name, self.options = ref_seq, alt_seq, reads, name, options

    trace = property(lambda self: self.options.trace)
    polish = property(lambda self: self.options.polish)
    junction = property(lambda self: self.options.junction)
    revote = property(lambda self: self.options.revote)


class Realigned(list):
    """The score list of a locus under `--realign` - the type's own driver's, as without the option - with `realign`: the payload
    of the last Score request the driver made whose answer was a list, None for a locus without one."""
    realign = None


def vapor_realign(options, name, driver, *args):
    """`--realign` for a DEL, INV, TANDUP or INS locus: the type's own driver runs as it is - its requests, its figure, its
    scores: the row's own columns - and the last Score request whose answer was a list is asked once more as a Realign request
    with the run's `options`, whichever branch made it (the short window and the junction window are both just a Score request).
    The request carries the locus's `name` where the options ask for traces."""
    gen = driver(*args)
    last = None
    try:
        req = next(gen)
        while True:
            try:
                ans = yield req
            except Exception as e:           # noqa: BLE001 - the executor's answer to a request may be an exception: the driver's to handle
                req = gen.throw(e)
                continue
            if isinstance(req, Score) and isinstance(ans, list):
                last = req
            req = gen.send(ans)
    except StopIteration as fin:
        scores = fin.value
    out = Realigned(scores if scores is not None else [])
    if last is not None:
        out.realign = yield Realign(last.ref_seq, last.alt_seq, last.reads, name if options.trace else None, options)
    return out


def vapor_simple_ins(num_reads_cff, plt_li, bam_in, ref, ins_pos, ins_seq, out_figure_name, POLARITY, phased=False):
    """vapor_simple_ins_Vapor, SF:1856-1893.  ins_pos is 'chrom_pos'."""
    if POLARITY == "+":
        ins_seq_2 = ins_seq
    elif POLARITY == "-":
        ins_seq_2 = _rc(ins_seq)
    else:
        raise UnboundLocalError("ins_seq_2")            # SF:1860-1861 leave it unbound
    flank = default_flank_length if len(ins_seq) > default_flank_length else len(ins_seq)
    chrom = "_".join(ins_pos.split("_")[:-1])
    pos_s = ins_pos.split("_")[-1]
    pos = int(pos_s)
    scores: List[float] = _scores(phased)
    reads = seqio.simple_chop_pacbio_read_simple_short(bam_in, [chrom, pos_s] + [pos + len(ins_seq)], flank, *((True,) if phased else ()))
    if len(reads) > num_reads_cff:
        if len(ins_seq) < 5000:
            ref_seq = seqio.ref_seq_readin(ref, chrom, pos - flank, pos + flank + len(ins_seq))
            k = yield from _window(ref_seq + ins_seq)
        else:
            ref_seq = seqio.ref_seq_readin(ref, chrom, pos - flank, pos + flank)
            k = yield from _window(ref_seq)
        if not k == "Error":
            # flank + ins_seq + flank, SF:1872 (both flanks lie inside the window just read)
            alt_seq = _cat(_within(ref_seq, pos - flank, seqio.ref_seq_readin(ref, chrom, pos - flank, pos), pos - flank),
                           (ins_seq_2, None, None),
                           _within(ref_seq, pos - flank, seqio.ref_seq_readin(ref, chrom, pos, pos + flank), pos))

            def few_n(x):                                   # SF:1878
                return float(x[0].count("N") + x[0].count("n")) / float(len(x[0])) < 0.1

            if phased:
                best = yield from _score_phased("s1", ref_seq, alt_seq, reads, k, scores, num_reads_cff, few_n)
            else:
                kept = [few_n(x) for x in reads]
                used = [x for x, f in zip(reads, kept) if f]
                res = (yield Score("s1", ref_seq, alt_seq, used, k)) if used else []
                best = _collect(res, reads, scores, keep=kept)
            if ins_seq_2.count("X") == len(ins_seq_2):
                yield Figure(scores, best, k, ref_seq, ref_seq[2:flank], out_figure_name)
            else:
                yield Figure(scores, best, k, ref_seq, alt_seq, out_figure_name)
    return scores


def vapor_simple_disdup(num_reads_cff, plt_li, bam_in, ref, sv_info, out_figure_name):
    """vapor_simple_disdup_Vapor, SF:1786-1854.  sv_info = [chrom, s, e, ins_chrom, ins_pos]."""
    sv_info[1:3] = [int(i) for i in sv_info[1:3]]
    dup_block = sv_info[:3]
    ins_point = [sv_info[3], int(sv_info[4])]
    flank = seqio.flank_length_calculate(dup_block)
    scores: List[float] = []
    bp = sorted([int(i) for i in sv_info[1:3] + [sv_info[4]]])
    ran = False
    if sv_info[0] == sv_info[3] and max(bp) - min(bp) < default_max_sv_test:
        ref_seq = seqio.ref_seq_readin(ref, sv_info[0], min(bp) - flank, max(bp) + flank)
        k = yield from _window(ref_seq)
        if not k == "Error":
            reads = seqio.simple_chop_pacbio_read_simple_short(
                bam_in, [sv_info[0]] + bp + [int(bp[-1]) + sv_info[2] - sv_info[1]], flank)
            if len(reads) > num_reads_cff:
                ran = True
                if sv_info[4] > sv_info[2]:
                    structure = ["a", "b", "a"]
                elif sv_info[4] < sv_info[1]:
                    structure = ["b", "a", "b"]
                else:
                    raise UnboundLocalError("alt_structure")  # SF:1803-1804: insert point inside the block
                w0 = min(bp) - flank                   # (every block lies inside the window just read: slices of it)
                parts = [_within(ref_seq, w0, seqio.ref_seq_readin(ref, sv_info[0], min(bp) - flank, min(bp)), w0)]
                a_seq = _within(ref_seq, w0, seqio.ref_seq_readin(ref, sv_info[0], bp[0], bp[1]), bp[0])
                b_seq = _within(ref_seq, w0, seqio.ref_seq_readin(ref, sv_info[0], bp[1], bp[2]), bp[1])
                for x in structure:
                    parts.append(a_seq if x == "a" else b_seq)
                parts.append(_within(ref_seq, w0, seqio.ref_seq_readin(ref, sv_info[0], max(bp), max(bp) + flank), max(bp)))
                alt_seq = _cat(*parts)
                k = yield from _window(alt_seq)
                if not k == "Error":
                    res = yield Score("s3", ref_seq, alt_seq, reads, k)
                    best = _collect(res, reads, scores)
                    yield Figure(scores, best, k, ref_seq, alt_seq, out_figure_name)
    if not ran:
        short = max(bp) - min(bp) < default_max_sv_test
        reads = seqio.simple_del_chop_pacbio_read_simple_short(bam_in, ins_point, flank)
        if len(reads) > num_reads_cff:
            ref_seq = seqio.ref_seq_readin(ref, ins_point[0], ins_point[1] - flank, ins_point[1] + flank)
            k = yield from _window(ref_seq)
            if not k == "Error":
                if short:
                    alt_seq = _cat((ref_seq, None, flank), (seqio.ref_seq_readin(ref, dup_block[0], dup_block[1], dup_block[2]), None, None),
                                   (ref_seq, -flank, None))
                else:
                    alt_seq = _cat((ref_seq, None, flank), (seqio.ref_seq_readin(ref, dup_block[0], dup_block[1], dup_block[1] + flank), None, None))
                k = yield from _window(alt_seq)
                if not k == "Error":
                    res = yield Score("s1" if short else "s2", ref_seq, alt_seq, reads, k)
                    best = _collect(res, reads, scores)
                    yield Figure(scores, best, k, ref_seq, alt_seq, out_figure_name)
    return scores


def vapor_dup_inv(num_reads_cff, plt_li, bam_in, ref, sv_info, out_figure_name):
    """vapor_dup_inv_VapoR, SF:1595-1665."""
    sv_info[1:3] = [int(i) for i in sv_info[1:3]]
    dup_block = sv_info[:3]
    ins_point = [sv_info[3], int(sv_info[4])]
    flank = seqio.flank_length_calculate(dup_block)
    scores: List[float] = []
    if sv_info[0] == sv_info[3]:
        bp = sorted(sv_info[1:3] + [sv_info[4]])
        ran = False
        if max(bp) - min(bp) < default_max_sv_test:
            ref_seq = seqio.ref_seq_readin(ref, sv_info[0], min(bp) - flank, max(bp) + flank)
            k = yield from _window(ref_seq)
            if not k == "Error":
                ran = True
                if sv_info[4] > sv_info[2]:
                    structure = ["a", "b", "a^"]
                elif sv_info[4] < sv_info[1]:
                    structure = ["b^", "a", "b"]
                else:
                    structure = ["a", "a^"]
                reads = seqio.simple_chop_pacbio_read_simple_short(
                    bam_in, [sv_info[0]] + bp + [bp[-1] + sv_info[2] - sv_info[1]], flank)
                if len(reads) > num_reads_cff:
                    w0 = min(bp) - flank
                    parts = [_within(ref_seq, w0, seqio.ref_seq_readin(ref, sv_info[0], min(bp) - flank, min(bp)), w0)]
                    a_seq = _within(ref_seq, w0, seqio.ref_seq_readin(ref, sv_info[0], bp[0], bp[1]), bp[0])
                    b_seq = _within(ref_seq, w0, seqio.ref_seq_readin(ref, sv_info[0], bp[1], bp[2]), bp[1])
                    for x in structure:
                        parts.append({"a": a_seq, "a^": _rcpart(a_seq), "b": b_seq, "b^": _rcpart(b_seq)}[x])
                    parts.append(_within(ref_seq, w0, seqio.ref_seq_readin(ref, sv_info[0], max(bp), max(bp) + flank), max(bp)))
                    alt_seq = _cat(*parts)
                    k = yield from _window(alt_seq)
                    if not k == "Error":
                        res = yield Score("s3", ref_seq, alt_seq, reads, k)
                        best = _collect(res, reads, scores)
                        yield Figure(scores, best, k, ref_seq, alt_seq, out_figure_name)
        if not ran:
            short = max(bp) - min(bp) < default_max_sv_test
            ref_seq = seqio.ref_seq_readin(ref, ins_point[0], ins_point[1] - flank, ins_point[1] + flank)
            k = yield from _window(ref_seq)
            if not k == "Error":
                reads = seqio.simple_del_chop_pacbio_read_simple_short(bam_in, ins_point, flank)
                if len(reads) > num_reads_cff:
                    if short:
                        alt_seq = _cat((ref_seq, None, flank), (seqio.ref_seq_readin(ref, dup_block[0], dup_block[1], dup_block[2]), None, None, True),
                                       (ref_seq, -flank, None))
                    else:
                        alt_seq = _cat((ref_seq, None, flank),
                                       (seqio.ref_seq_readin(ref, dup_block[0], dup_block[2] - flank, dup_block[2]), None, None, True))
                    k = yield from _window(alt_seq)
                    if not k == "Error":
                        res = yield Score("s1" if short else "s2", ref_seq, alt_seq, reads, k)
                        best = _collect(res, reads, scores)
                        yield Figure(scores, best, k, ref_seq, alt_seq, out_figure_name)
    return scores


def vapor_long_del_inv(num_reads_cff, plt_li, bam_in, ref, sv_info, out_figure_name):
    """vapor_long_del_inv, SF:1667-1688.  sv_info = [[chrom, s, e, 'del'], [chrom, s, e, 'inv']]."""
    scores: List[float] = []
    flank = 500
    ref_seq = seqio.ref_seq_readin(ref, sv_info[0][0], sv_info[0][1] - flank, sv_info[1][1] + flank)
    k = yield from _window(ref_seq)
    if not k == "Error":
        alt_seq = _cat((ref_seq, None, flank), (seqio.ref_seq_readin(ref, sv_info[1][0], sv_info[1][2] - flank, sv_info[1][2]), None, None, True))
        k = yield from _window(alt_seq)
        if not k == "Error":
            reads = seqio.simple_del_chop_pacbio_read_simple_short(bam_in, sv_info[0], flank)
            if len(reads) > num_reads_cff:
                res = yield Score("s2", ref_seq, alt_seq, reads, k)
                best = _collect(res, reads, scores)
                yield Figure(scores, best, k, ref_seq, alt_seq, out_figure_name)
    return scores


def vapor_del_inv(num_reads_cff, plt_li, bam_in, ref, sv_info, out_figure_name):
    """vapor_del_inv_Vapor, SF:1557-1593.  sv_info = ordered [[chrom, s, e, 'del'|'inv'], ...]."""
    sv_block = [sv_info[0][0], sv_info[0][1], sv_info[-1][2]]
    flank = seqio.flank_length_calculate(sv_block)
    scores: List[float] = []
    if sv_info[1][1] - sv_info[0][2] < 100:
        if sv_block[2] - sv_block[1] < default_max_sv_test:
            ref_seq = seqio.ref_seq_readin(ref, sv_block[0], sv_block[1] - flank, sv_block[2] + flank)
            k = yield from _window(ref_seq)
            if not k == "Error":
                parts = [(ref_seq, None, flank)]
                for x in sv_info:
                    if x[-1] == "del":
                        continue
                    elif x[-1] == "inv":
                        parts.append(_rcpart(_within(ref_seq, sv_block[1] - flank, seqio.ref_seq_readin(ref, x[0], x[1], x[2]), x[1])))
                parts.append((ref_seq, -flank, None))
                alt_seq = _cat(*parts)
                k = yield from _window(alt_seq)
                if not k == "Error":
                    reads = seqio.simple_chop_pacbio_read_simple_short(
                        bam_in, sv_block[:2] + [sv_block[1] + len(alt_seq) - 2 * flank], flank)
                    if len(reads) > num_reads_cff:
                        res = yield Score("s1", ref_seq, alt_seq, reads, k)
                        best = _collect(res, reads, scores)
                        yield Figure(scores, best, k, ref_seq, alt_seq, out_figure_name)
                    else:
                        if len(sv_info) == 2 and [i[-1] for i in sv_info] == ["del", "inv"]:
                            # SF:1585 calls vapor_long_del_inv with four arguments
                            raise TypeError("vapor_long_del_inv() missing 2 required positional arguments: "
                                            "'sv_info' and 'out_figure_name'")
        else:
            if len(sv_info) == 2 and [i[-1] for i in sv_info] == ["del", "inv"]:
                scores = yield from vapor_long_del_inv(num_reads_cff, plt_li, bam_in, ref, sv_info, out_figure_name)
    else:
        for sub in sv_info:
            if "del" in sub or "inv" in sub:
                # SF:1591-1592 call the simple drivers with four arguments
                raise TypeError("vapor_simple_%s_Vapor() missing 2 required positional arguments: "
                                "'sv_info' and 'out_figure_name'" % ("del" if "del" in sub else "inv"))
    return scores


# ------------------------------------------------------------------------------------------
# complex structures written as letter strings (SVelter style): 'ab_ab' -> 'b_b^' etc.
# ------------------------------------------------------------------------------------------

def letter_split(let):
    """SF:1013-1019: 'c^ba' -> ['c^', 'b', 'a']."""
    out = []
    for x in let:
        if not x == '^':
            out.append(x)
        else:
            out[-1] += x
    return out


def list_unify(items):
    """SF:1021-1025."""
    out = []
    for i in items:
        if i not in out:
            out.append(i)
    return out


def block_subsplot(bp_list, chromos):
    """SF:147-153: ['chr1', '10', '20', 'chr2', '5', '9'] -> [['chr1', 10, 20], ['chr2', 5, 9]]."""
    out = []
    for x in bp_list:
        if x not in chromos:
            out[-1].append(int(x))
        else:
            out.append([x])
    return out


def bp_to_chr_hash(bps, chromos, flank_length=500):
    """SF:98-114: letters a, b, ... for consecutive blocks, '-' / '+' for the flanks (with the
    reference's mix of int and str coordinates)."""
    groups = []
    for i in bps:
        if i in chromos:
            groups.append([i])
        else:
            groups[-1].append(i)
    out = {}
    rec = -1
    for k1 in groups:
        for k2 in range(len(k1[2:])):
            rec += 1
            out[chr(97 + rec)] = [k1[0], k1[k2 + 1], k1[k2 + 2]]
    last = out[sorted(out.keys())[-1]]
    out['+'] = [last[0], last[2], str(int(last[2]) + flank_length)]
    out['-'] = [out['a'][0], str(int(out['a'][1]) - flank_length), int(out['a'][1])]
    return out


def block_around_check(alt_allele, ref_allele):
    """SF:91-96: junctions of the alt allele that the ref allele does not have."""
    al = ['-'] + letter_split(alt_allele) + ['+']
    rl = ['-'] + letter_split(ref_allele) + ['+']
    n = len(letter_split(alt_allele)) + 1
    alt_j = [al[j:j + 2] for j in range(n)]
    ref_j = [rl[j:j + 2] for j in range(n)]
    return [i for i in alt_j if i not in ref_j]


def vapor_cannot_classify(num_reads_cff, plt_li, bam_in, ref, sv_info, out_figure_name):
    """vapor_CANNOT_CLASSIFY_VapoR, SF:1490-1555.
    sv_info = ['ab_ab', 'b_b^', 'chr7', '70955990', '70961199', '70973901']."""
    ref_sv = sv_info[0].split('_')
    alt_sv = list_unify([i for i in sv_info[1].split('_') if i not in ref_sv])
    chromos = seqio.chromos_readin(ref)
    bp_info = block_subsplot(sv_info[2:], chromos)
    flank = max([seqio.flank_length_calculate(i) for i in bp_info])
    scores: List[float] = []
    ran = False
    if len(bp_info) == 1:
        b0 = bp_info[0]
        if b0[-1] - b0[1] < default_max_sv_test:
            ref_seq = seqio.ref_seq_readin(ref, b0[0], b0[1] - flank, b0[-1] + flank)
            k = yield from _window(ref_seq)
            if not k == "Error":
                reads = seqio.simple_chop_pacbio_read_simple_short(bam_in, b0, flank)
                let_hash = bp_to_chr_hash(b0, chromos, flank)
                if len(reads) > num_reads_cff:
                    ran = True
                    let_seq = {}
                    for i in list(let_hash.keys()):
                        let_seq[i] = seqio.ref_seq_readin(ref, let_hash[i][0], int(let_hash[i][1]), int(let_hash[i][-1]))
                    for alt_allele in alt_sv:
                        parts = [(ref_seq, None, flank)]
                        for i in letter_split(alt_allele):
                            blk = _within(ref_seq, b0[1] - flank, let_seq[i[0]], int(let_hash[i[0]][1]))
                            parts.append(blk if '^' not in i else _rcpart(blk))
                        parts.append((ref_seq, -flank, None))
                        alt_seq = _cat(*parts)
                        k = yield from _window(alt_seq)
                        if not k == "Error":
                            repeated = max([alt_allele.count(i) for i in alt_allele] + [0]) > 1
                            res = yield Score("s3" if repeated else "s1", ref_seq, alt_seq, reads, k)
                            best = _collect(res, reads, scores)
                            parts = out_figure_name.split('.')
                            yield Figure(scores, best, k, ref_seq, alt_seq,
                                         '.'.join(parts[:-1] + [ref_sv[0] + '.vs.' + alt_allele, parts[-1]]))
        if not ran:
            for alt_allele in alt_sv:
                juncs = block_around_check(alt_allele, ref_sv[0])
                let_hash = bp_to_chr_hash(b0, chromos, flank)
                for jun in juncs:
                    ha, hb = let_hash[jun[0][0]], let_hash[jun[1][0]]
                    if '^' not in jun[0]:
                        ref_a = seqio.ref_seq_readin(ref, ha[0], ha[2] - flank, ha[2] + flank)
                    else:
                        ref_a = _rc(seqio.ref_seq_readin(ref, ha[0], ha[1] - flank, ha[1] + flank))
                    if '^' not in jun[1]:
                        ref_b = seqio.ref_seq_readin(ref, hb[0], hb[1] - flank, hb[1] + flank)
                    else:
                        ref_b = _rc(seqio.ref_seq_readin(ref, hb[0], hb[2] - flank, hb[2] + flank))
                    k = yield from _window(ref_a + ref_b)
                    if not k == "Error":
                        alt_seq = ref_a[-flank:] + ref_b[:flank]
                        k = yield from _window(alt_seq)
                        if not k == "Error":
                            where = [ha[0], ha[2]] if '^' not in jun[0] else [ha[0], ha[1]]
                            reads = seqio.simple_del_chop_pacbio_read_simple_short(bam_in, where, flank)
                            if len(reads) > 0:
                                res = yield Score("s2", ref_a, alt_seq, reads, k)
                                _collect(res, reads, scores)
    return scores

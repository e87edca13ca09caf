"""`vapor bed | vcf | svelter | ins` - the reference's command line (vapor_vali/vapor:287-496) on the HIP path.

Same sub-commands, same flags, same output files and rows.  What differs is the schedule: the
reference scores one locus at a time; here every locus becomes a driver generator
(vapor_amd.drivers) and `pipeline.run_batch` sends the pending dot plots of a whole chunk of loci
to the GPU together.  With more than one rank (torchrun), loci are sharded across the GPUs of
the node and the per-locus rows are all-gathered (vapor_amd.dist).

Extra flags (not in the reference): --no-figures (skip the recurrence-plot PNGs),
--chunk (loci per device batch), --bnd (vcf: score breakend records as well), --refine M[:T] (bed, vcf: score a
grid of candidate breakpoints within M bp of every short DEL / INV / TANDUP call and report the best),
--phased (bed, vcf: read the HP and PS tags of a haplotagged BAM and score the reads of each haplotype of a DEL / INV / TANDUP /
INS call beside the pooled list; appends VaPoR_PS, VaPoR_PGT, VaPoR_PGQ and QS / GS / Rec per haplotype; not
together with --refine), --both-ends (bed, vcf: every junction branch - long DEL / INV, TANDUP, breakends - is scored from both of
its sides, with right-anchored reads; appends the VaPoR_BE_* columns; not together with --refine or --phased),
--phase-vcf FILE [--phase-sample NAME] (bed, vcf: --phased for a BAM that is NOT haplotagged - every read's haplotype and phase
set come from its bases at the phased heterozygous SNVs of FILE; the HP / PS tags of the BAM are not read),
--min-mapq Q and --exclude-flags F (every sub-command, with every other option): a record is filtered iff
MAPQ < Q or (FLAG & F) != 0 - `samtools view -q Q -F F` - and a filtered record is treated as if it were not in the file, on
every read route; the default, 0 and 0, filters nothing.  --dedup-qname (every sub-command, with every other option; DESIGN.md
§4.18): records with one QNAME are one molecule - among the kept records of one (file, region, anchor kind) one survives, the
first that is neither secondary (0x100) nor supplementary (0x800), else the first, and the others are treated as if they were
not in the file; with --both-ends the pooled VaPoR_BE_* columns count a molecule once across the views.  It adds no column.
--depth (bed, vcf): read depth inside every DEL and TANDUP call against the depth of its 1 kb flanks, a second
line of evidence beside the dot plots; appends VaPoR_DP_IN, VaPoR_DP_FL, VaPoR_DFC and VaPoR_DSUP; the row's own columns are
the plain run's; not together with --refine, --phased, --phase-vcf or --both-ends.
--signatures (bed, vcf): split-read and CIGAR evidence per DEL, TANDUP, INV and INS call - the alignments clipped
at its breakpoints, those that carry it as a D, N or I, and the modal breakpoints they give; appends VaPoR_SIG_L, VaPoR_SIG_R,
VaPoR_SIG_CG, VaPoR_SIG_N, VaPoR_SIG_POS and VaPoR_SIG_END; the row's own columns are the plain run's; not together with another
of these modes.
--links (bed, vcf): split reads joined through their SA tags, per DEL, TANDUP and INV call and per breakend of
--bnd - the alignments clipped at a breakpoint whose SA tag names a piece at the call's other breakpoint, on the strand the event
gives it; those that are split but go elsewhere; and the modal coordinates the linked pieces name; appends VaPoR_LNK_L,
VaPoR_LNK_R, VaPoR_LNK_N, VaPoR_LNK_OL, VaPoR_LNK_OR, VaPoR_LNK_POS and VaPoR_LNK_END; the row's own columns are the plain
run's; not together with another of these modes.
--support (bed, vcf): alt and ref alignments per DEL, TANDUP, INV and INS call - the records that carry the event
and the records that run straight through a breakpoint as the reference does - with the allele fraction and the genotype the two
numbers give; appends VaPoR_SUP_ALT, VaPoR_SUP_REF, VaPoR_SUP_REFL, VaPoR_SUP_REFR, VaPoR_SUP_COVL, VaPoR_SUP_COVR, VaPoR_SUP_VAF,
VaPoR_SUP_GT and VaPoR_SUP_GQ; the row's own columns are the plain run's; not together with another of these modes.

--refine, --phased (with --phase-vcf), --both-ends, --depth, --signatures, --links and --support each append columns to every row and exclude one another: a run has one
mode (vapor_amd.modes) or none, built once in _main and handed as one argument to bed_jobs / vcf_jobs (which
driver a locus takes), score_jobs (the payload gathered into Job.extra), the table writer and SF.vcf_vapor_modify.  An option
that adds columns is a module with INFO, COLUMNS, pack, unpack and columns_many, a Mode made of it, and its branch in _simple_job.
"""
# (The text above is also `vapor --help`'s description.)  The four evidence modes - --depth, --signatures, --links, --support - have
# one chunk hook between them, _evidence_payloads, which reads a chunk's regions through the rule module's reader surface
# (DESIGN.md 4.16), and the parser refuses every pair of mode options from one list and one table (MODE_OPTIONS, PAIR_REASONS).
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional

from . import dist as vdist
from . import depth, drivers, links, modes, pipeline, signature, support
from . import simple_function as SF
from .finish import result_organize_ins, row_tail


# ------------------------------------------------------------------------------------------
# input parsers (SURVEY.md component #10)
# ------------------------------------------------------------------------------------------

def bed_info_readin(bed_input, out_path):
    """vapor_vali/vapor:22-50: rows are chr start end SVID TYPE [INS sequence]."""
    out_path = SF.path_modify(out_path)
    SF.path_mkdir(out_path)
    out = []
    with open(bed_input) as fin:
        for line in fin:
            pin = line.strip().split()
            t = pin[4]
            if 'DUP' in t or 'duplication' in t:
                out.append([pin[0]] + [int(i) for i in pin[1:3]] + [pin[3]] + ['a/a', 'a/aa'])
            elif 'DEL' in t or 'deletion' in t:
                out.append([pin[0]] + [int(i) for i in pin[1:3]] + [pin[3]] + ['a/a', '/a'])
            elif 'INV' in t or 'inversion' in t:
                out.append([pin[0]] + [int(i) for i in pin[1:3]] + [pin[3]] + ['a/a', 'a/a^'])
            elif 'INS' in t or 'ALU' in t or 'HERVK' in t or 'LINE1' in t or 'SVA' in t or 'insertion' in t:
                if len(pin) > 5:
                    out.append([pin[0], int(pin[1]), int(pin[2]), pin[3], pin[5], 'INS'])
                elif '_' in t:
                    v = t.split('_')[1]
                    out.append([pin[0], int(pin[1]), int(pin[2]), pin[3], int(v) if v.isdigit() else v, 'INS'])
    return out


def block_reorganize(block_hash):
    """vapor_vali/vapor:83-97: blocks of one chromosome ordered by start, duplicates dropped."""
    if len(block_hash) == 1:
        for k1 in block_hash:
            start = [i[1] for i in block_hash[k1]]
            order = [start.index(i) for i in sorted(start)]
            out = []
            for b in [block_hash[k1][i] for i in order]:
                if b not in out:
                    out.append(b)
            return out
    return 'error'


def del_inv_interprete(pin):
    """vapor_vali/vapor:99-111: del=chr:s-e / inv=chr:s-e INFO entries."""
    out = {}
    for x in pin[7].split(';'):
        for tag, name in (('del=', 'del'), ('DEL=', 'del'), ('inv=', 'inv'), ('INV=', 'inv')):
            if tag in x:
                v = x.split('=')[1]
                blk = [v.split(':')[0]] + [int(i) for i in v.split(':')[1].split('-')]
                out.setdefault(blk[0], []).append(blk + [name])
                break
    return block_reorganize(out)


def dup_inv_interprete(pin):
    """vapor_vali/vapor:113-125."""
    seg = [pin[0], int(pin[1])]
    ins = []
    for x in pin[7].split(';'):
        if 'END=' in x:
            seg.append(int(x.split('=')[1]))
        if 'insert_point' in x or 'INSERT_POINT' in x:
            ins = x.split('=')[1].split(':')
    if len(ins) > 1:
        return seg + [ins[0], int(ins[1])]
    return 'error'


def vcf_list_readin(file_in, bnd_ref=None, both_ends=False):
    """vapor_vali/vapor:127-202: records bucketed by type in first-seen order, plus
    {file line index: key} for the INFO rewrite.  `bnd_ref` (the reference FASTA, `vapor vcf --bnd`): breakend records are
    read as well, into a 'BND' bucket that comes last (bnd_view); without it they take the reference's last branch."""
    out = {}
    rec_hash = {}
    bnd = _BndReader(bnd_ref, both_ends) if bnd_ref is not None else None
    rec = -1
    # `x not in out[T]` of the reference scans the bucket's list (every record against every earlier one of its type: minutes
    # on a call set of 10^5); the same test from a set of the entries as tuples beside each list
    seen = {}

    def key(x):
        return tuple(key(i) if isinstance(i, list) else i for i in x)

    def new(bucket, probe, item=None):
        """`probe not in out[bucket]`, and if so the item (default: the probe) appended."""
        ks = seen.setdefault(bucket, set())
        if key(probe) in ks:
            return False
        item = probe if item is None else item
        out[bucket].append(item)
        ks.add(key(item))
        return True
    with open(file_in) as fin:
        for line in fin:
            rec += 1
            pin = line.strip().split()
            if pin[0][0] == '#':
                continue
            pin[7] = pin[7].replace('MERGE_TYPE=', 'SVTYPE=')
            t = SF.svtype_extract(pin)
            pos = SF.chr_start_end_extract(pin)

            if t in ['del', 'DEL', 'deletion']:
                out.setdefault('DEL', [])
                if new('DEL', pos):
                    rec_hash[rec] = ':'.join([str(i) for i in pos] + ['DEL'])
            elif t in ['inv', 'INV', 'inversion']:
                out.setdefault('INV', [])
                if new('INV', pos):
                    rec_hash[rec] = ':'.join([str(i) for i in pos] + ['INV'])
            elif t in ['ins', 'INS', 'insertion', 'LINE1', 'SVA', 'ALU', 'HERVK']:
                sv_len = int(SF.sv_len_extract(pin))
                seq = SF.sv_seq_extract(pin)
                if sv_len > 0:
                    out.setdefault('INS', [])
                    if new('INS', pos, pos[:2] + [sv_len, seq]):     # (the probe has three fields, the entries four: never a duplicate)
                        rec_hash[rec] = ':'.join([str(i) for i in pos[:2] + [sv_len]] + ['INS'])
            elif t in ['disdup', 'DISDUP', 'dis-dup']:
                ip = SF.sv_insert_point_define(pin)
                out.setdefault('DISDUP', [])
                if new('DISDUP', pos, pos + ip):
                    rec_hash[rec] = ':'.join([str(i) for i in pos + ip] + ['DISDUP'])
            elif t in ['DEL_INV', 'del_inv']:
                out.setdefault('DEL_INV', [])
                info = del_inv_interprete(pin)
                if not info == 'error' and new('DEL_INV', info):
                    rec_hash[rec] = ':'.join(['_'.join([str(i) for i in j]) for j in info] + ['DEL_INV'])
            elif t in ['DUP_INV', 'dup_inv']:
                out.setdefault('DUP_INV', [])
                info = dup_inv_interprete(pin)
                if not info == 'error' and new('DUP_INV', info):
                    rec_hash[rec] = ':'.join([str(i) for i in info + ['DUP_INV']])
            elif t in ['tandup', 'TANDUP', 'DUP']:
                out.setdefault('TANDUP', [])
                if new('TANDUP', pos):
                    rec_hash[rec] = ':'.join([str(i) for i in pos] + ['TANDUP'])
            elif t in ['CNV', 'CSV', 'CPX']:
                continue
            else:
                if bnd is not None and t in ('BND', 'bnd') and 'Other=' not in pin[7] and 'OTHER=' not in pin[7]:
                    bnd.take(rec, pin, rec_hash)
                    continue
                if 'Other=' in pin[7]:
                    info = [i for i in pin[7].split(';') if i[:6] == 'Other=']
                elif 'OTHER=' in pin[7]:
                    info = [i for i in pin[7].split(';') if i[:6] == 'OTHER=']
                else:
                    continue
                o = info[0].split('=')[1].split('_')
                item = ['_'.join(i.split('/')) for i in o[:2]] + o[2].split(':')
                out.setdefault('Other', [])
                if new('Other', item):
                    rec_hash[rec] = ':'.join([str(i) for i in item + ['CANNOT_CLASSIFY']])
    if bnd is not None and bnd.loci:
        out['BND'] = bnd.loci
    return [out, rec_hash]


# ------------------------------------------------------------------------------------------
# breakends (`vapor vcf --bnd`; not in the reference: DESIGN.md §7)
# ------------------------------------------------------------------------------------------

def bnd_alt(alt: str):
    """The ALT of a breakend record in one of the four VCF 4.x forms: (CT, B, q, inserted bases), or the reason it is not one.
    `t[B:q[` 3to5 and `t]B:q]` 3to3 insert t[1:], `]B:q]t` 5to3 and `[B:q[t` 5to5 insert t[:-1] (t: the mate's REF base and
    the bases inserted between the two pieces)."""
    if ',' in alt:
        return 'several ALTs'
    if '[' not in alt and ']' not in alt:
        return 'single breakend' if len(alt) >= 2 and (alt[0] == '.' or alt[-1] == '.') else 'malformed ALT'
    c0, c1 = alt[0], alt[-1]
    if c0 in '[]':
        j = alt.find(c0, 1)
        if j < 0:
            return 'malformed ALT'
        inner, t = alt[1:j], alt[j + 1:]
        ct, ins = ('5to3' if c0 == ']' else '5to5'), t[:-1]
    elif c1 in '[]':
        i = alt.find(c1)
        if i == len(alt) - 1:
            return 'malformed ALT'
        t, inner = alt[:i], alt[i + 1:-1]
        ct, ins = ('3to5' if c1 == '[' else '3to3'), t[1:]
    else:
        return 'malformed ALT'
    b, _, q = inner.rpartition(':')
    if not (t and t.isascii() and t.isalpha() and b and '[' not in b and ']' not in b and q.isascii() and q.isdigit()
            and int(q) >= 1):
        return 'malformed ALT'
    return ct, b, int(q), ins


def bnd_view(chrom: str, pos: int, alt: str, both_ends: bool = False):
    """The scored view of a breakend record at chrom:pos - [A, p, B, q, CT, inserted bases] with CT '3to5' or '3to3', the
    left-hand piece's reads clipped on the right at A:p - or the reason it is skipped.  A `5to3` record is scored as its mirror
    `t[A:p[` at B:q (the same junction); a `5to5` record has no such view - with both_ends (`--both-ends`: right-anchored
    reads) it is taken with CT '5to5'."""
    got = bnd_alt(alt)
    if isinstance(got, str):
        return got
    ct, b, q, ins = got
    if ct == '5to5' and both_ends:
        return [chrom, int(pos), b, q, ct, ins]
    if ct == '5to5':
        return '5to5 junction: its reads are clipped on the left, which the read model (SF:339-354) does not take'
    if ct == '5to3':
        return [b, q, chrom, int(pos), '3to5', ins]
    return [chrom, int(pos), b, q, ct, ins]


def bnd_key(view) -> str:
    """A:p:B:q:CT:BND of a scored view (a `5to3` record and its `3to5` mate share it)."""
    return ':'.join([str(i) for i in view[:5]] + ['BND'])


def _mate_id(info: str):
    for x in info.split(';'):
        if x[:7] == 'MATEID=' or x[:8] == 'MATE_ID=':
            return x.split('=', 1)[1]
    return None


class _BndReader:
    """vcf_list_readin's breakend records: one locus per key, in first-seen order (as the reference de-duplicates sv_pos);
    mates (MATEID / MATE_ID) are scored once, at the record that comes first, and every record taken carries its locus's key
    in rec_hash, so that both mates get the annotation.  A skipped record gets one line on stderr and no row."""

    def __init__(self, ref, both_ends=False):
        from . import seqio
        self.both_ends = both_ends
        self.chromos = seqio.chromos_readin(ref)
        self.loci, self.keys = [], set()
        self.by_id, self.by_mate = {}, {}

    def take(self, rec, pin, rec_hash):
        alt = pin[4] if len(pin) > 4 else ''
        view = bnd_view(pin[0], int(pin[1]), alt, True) if self.both_ends else bnd_view(pin[0], int(pin[1]), alt)
        if not isinstance(view, str):
            miss = [c for c in (view[0], view[2]) if c not in self.chromos]
            if miss:
                view = 'contig %s not in the .fai' % miss[0]
        if isinstance(view, str):
            print('vapor vcf --bnd: record %s:%s %s skipped: %s' % (pin[0], pin[1], alt, view), file=sys.stderr)
            return
        rid, mate = pin[2] if len(pin) > 2 else '.', _mate_id(pin[7])
        key = self.by_id.get(mate) if mate else None
        if key is None and rid != '.':
            key = self.by_mate.get(rid)
        if key is None:
            key = bnd_key(view)
            if key not in self.keys:
                self.keys.add(key)
                self.loci.append(view)
        rec_hash[rec] = key
        if rid != '.':
            self.by_id.setdefault(rid, key)
        if mate:
            self.by_mate.setdefault(mate, key)


# ------------------------------------------------------------------------------------------
# jobs
# ------------------------------------------------------------------------------------------

class Job:
    """One output row: how to score it (a driver call, a generator factory, or fixed scores) and how to
    write it.  `cost`: what the locus is expected to take (microseconds, `job_cost`), for the shares of the ranks."""
    __slots__ = ("key", "make", "fixed", "row_prefix", "label", "cost", "spec", "ctx", "call", "extra", "bnd")

    def __init__(self, key, make=None, fixed=None, row_prefix=None, label=None, cost=None, spec=None, ctx=None, call=None, bnd=None):
        # `call` = (driver, its arguments ..): `make` is that call, and a mode's chunk hook can make it again over other reads
        if call is not None:
            make = lambda: call[0](*call[1:])               # noqa: E731
        self.key, self.make, self.fixed, self.row_prefix, self.label, self.call = key, make, fixed, row_prefix, label, call
        # the four simple types also say WHAT they are - (type, chrom, start, end, ins_seq) and (num_reads_cff, bam, ref) - so
        # that a chunk of them can take the array route (vapor_amd.fastpath); `make` stays the driver's own route
        self.spec, self.ctx = spec, ctx
        # a breakend says what it is apart from them - (its scored view, (num_reads_cff, bam, ref)) - for a mode's chunk hook
        # (`--links`); spec and ctx stay None: a breakend is not for the array route
        self.bnd = bnd
        self.extra = None              # after scoring under a mode (vapor_amd.modes): the locus's payload - refine.Refined.info,
                                       # phase.Phased.phase or drivers.BothEnds.views -, None for a locus without one
        self.cost = cost if cost is not None else (COST_FIXED_US if make is None else COST_HOST_US)


# What a locus costs, for the ranks' shares (greedy longest-processing-time on the estimated cost, not round-robin
# by index - spans run from 50 bp to 21 kb windows, vapor_vali/vapor:334-367).  Three terms, priced on one MI355X box with its
# host (tools/fit_job_cost.py, profiles/r04_job_cost_fit.json): the per-locus interpreter work; what scales with the bases
# handled (reads extracted, trimmed, staged, uploaded and packed; windows read and uploaded); and the device term SURVEY 8e
# names, n_reads x Lr x (La_ref + La_alt) nominal cells, at the rate the kernels go through them.
COST_FIXED_US = 0.5            # a row without device work (an SV below 50 bp in vcf mode)
COST_HOST_US = 40.0            # generator protocol, extraction call, tables, row (fit: 39-48)
COST_PER_KBASE_US = 0.35       # per 1 000 bases of reads and windows handled (fit: 0.27-0.64)
COST_PER_GCELL_US = 0.25       # per 1e9 nominal read-bp x window-bp cells: the kernels' own rate (cfg2: 8.0e11 cells per 0.178 ms
                               # pass); too small beside the host terms for the fit to see
COST_XMEANS_US = 500.0         # a tandem duplication's alt window always meets the X-means branch of the repeat check
                               # (sklearn / scipy on the host workers: 290-1 360 us per locus measured, by no simple rule of the span)
_READS_KEPT = 20               # minimize_pacbio_read_list keeps at most 20 reads (SF:1091-1102)


def job_cost(svtype: str, span: int, extra: int = 0, candidates: int = 1, views: int = 1) -> float:
    """Expected cost of one locus in microseconds from its type and span alone (windows as the drivers cut them, SURVEY.md
    3.2): `span` = end - start (INS: the inserted length; complex types: the whole region), `extra` = the duplicated block of
    DISDUP / DUP_INV, `candidates` = the alleles scored on the window (`--refine`: every read meets the window once and every
    candidate allele once), `views` = the views of the locus's junction (`--both-ends`: 2, 4 for an INV).  An estimate for
    balancing shares - nothing depends on its accuracy but the ranks' idle time."""
    span = max(int(span), 0)
    f = min(500, span) if span > 0 else 500
    short = span < drivers.default_max_sv_test
    if svtype == 'BND':                     # a breakend: the windows of a long deletion's junction (drivers.vapor_bnd)
        lr, la = 2 * 500, 4 * 500
    elif svtype == 'DEL':
        lr, la = 2 * f, ((span + 2 * f) + 2 * f if short else 4 * f)
    elif svtype == 'INV':
        lr, la = (span + 2 * f, 2 * (span + 2 * f)) if short else (2 * f, 4 * f)
    elif svtype == 'TANDUP':
        lr, la = (2 * span + 2 * f, (span + 2 * f) + (2 * span + 2 * f)) if short else (2 * f, 4 * f)
    elif svtype == 'INS':
        lr, la = span + 2 * f, (2 * f + (span if span < 5000 else 0)) + (span + 2 * f)
    else:                                   # DISDUP, DUP_INV, DEL_INV, Other: the whole region when it is short
        lr, la = (span + extra + 2 * f, (span + 2 * f) + (span + extra + 2 * f)) if short else (2 * f, 4 * f)
    bases = _READS_KEPT * lr + la
    cells = _READS_KEPT * lr * la
    if candidates > 1:                      # (la = window + one allele: the other candidates' alleles are about that allele's size)
        cells += _READS_KEPT * lr * (candidates - 1) * (la / 2.0)
    xmeans = COST_XMEANS_US if (svtype == 'TANDUP' and short) else 0.0
    if views > 1:                           # (`--both-ends`: every extra view is a junction window pair with reads of its own)
        bases += (views - 1) * (_READS_KEPT * 2 * f + 4 * f)
        cells += (views - 1) * _READS_KEPT * 2 * f * 4 * f
    return COST_HOST_US + COST_PER_KBASE_US * bases / 1e3 + COST_PER_GCELL_US * cells / 1e9 + xmeans


def _views_n(name, span) -> int:
    """The views `--both-ends` may score for a locus (job_cost): the junction branch of a long call, 1 for a short one."""
    if name == 'BND':
        return 2
    if span < drivers.default_max_sv_test:
        return 1
    return 4 if name == 'INV' else 2


_SIMPLE = {'DEL': drivers.vapor_simple_del, 'INV': drivers.vapor_simple_inv, 'TANDUP': drivers.vapor_simple_tandup}


def _simple_job(name, info, key, fig, row_prefix, label, plt_li, ctx, mode, with_mode=True) -> Job:
    """The job of a DEL / INV / TANDUP record `info` = [chrom, start, end].  Plain and `--phased`: the type's own driver, with
    its array-route description.  `--refine`: drivers.vapor_refine (which leaves a locus it cannot refine to the type's own
    driver), within the record's CIPOS / CIEND where the mode has them.  `--both-ends`: drivers.vapor_both_ends.  `--realign`:
    drivers.vapor_realign around the type's own driver, on the drivers' route.  `with_mode` False: a record that these drivers do
    not take goes the plain way."""
    n_cff, bam_in, ref = ctx
    span = info[2] - info[1]
    spec = (name, info[0], info[1], info[2], None)       # (None below: the locus is not for the array route)
    kind = mode.name if mode is not None and with_mode else None
    if kind == 'refine':
        from . import refine as rf
        (m, t), ci = mode.margin_step, mode.ci_of.get(key, (None, None))
        call = (drivers.vapor_refine, name, n_cff, plt_li, bam_in, ref, info, fig, m, t, ci[0], ci[1])
        cost, spec = job_cost(name, span, candidates=len(rf.candidates(m, t, info[1], info[2], ci[0], ci[1]))), None
    elif kind == 'both-ends':
        # (a call that may reach its junction branch takes the drivers' route: the array route has no extra views; a short
        # DEL never reaches it and stays where it was)
        if name != 'DEL' or not span < drivers.default_max_sv_test:
            spec = None
        call = (drivers.vapor_both_ends, name, n_cff, plt_li, bam_in, ref, info, fig)
        cost = job_cost(name, span, views=_views_n(name, span))
    elif kind == 'realign':
        # (every read meets both alleles once more, in a band: about the cost of the locus again; the array route has no second pass)
        call = _realign_call(mode, key, (_SIMPLE[name], n_cff, plt_li, bam_in, ref, info, fig, False))
        cost, spec = 2 * job_cost(name, span), None
    else:
        call = (_SIMPLE[name], n_cff, plt_li, bam_in, ref, info, fig, mode is not None and mode.phased)
        cost = job_cost(name, span)
    return Job(key, None, None, row_prefix, label, cost, spec, ctx, call)


def _realign_call(mode, key, call):
    """`call` = (driver, *args) under `--realign`: drivers.vapor_realign around it, with the mode's options and the locus's key -
    the name of its Realign request where the options ask for traces."""
    return (drivers.vapor_realign, mode.options, key) + call


def _ins_job(call, cost, spec, mode, key=None):
    """(call, cost, array-route description) of an INS locus: as given, and under `--realign` drivers.vapor_realign around the
    call, about twice its cost, on the drivers' route (no description), as _simple_job has it for the other three types."""
    if mode is not None and mode.name == 'realign':
        return _realign_call(mode, key, call), 2 * cost, None
    return call, cost, spec


def bed_jobs(bed_info, num_reads_cff, bam_in, ref, out_path, sample_name, mode=None) -> List[Job]:
    """The loop of vapor_vali/vapor:334-367.  `mode` (vapor_amd.modes): the run's extra-columns option, None without one -
    _simple_job for the DEL, INV and TANDUP loci, and under `--phased` the INS driver reads the tags as well (the array
    route takes the option from score_jobs)."""
    jobs = []
    plt_li = 0
    ctx = (num_reads_cff, bam_in, ref)
    phased = mode is not None and mode.phased
    for x in bed_info:
        tag = x[-1]
        if tag in ['a/', '/a', '/', 'DEL']:
            name = 'DEL'
        elif tag in ['a/a^', 'a^/a', 'a^/a^', 'INV']:
            name = 'INV'
        elif tag in ['INS']:
            key = ':'.join([str(i) for i in x[:-3] + ['INS']])
            plt_li += 1
            ins_pos = '_'.join([str(i) for i in x[:2]])
            ins_seq = ''.join(['X' for _ in range(x[4])]) if type(x[4]) == type(4) else x[4]
            fig = out_path + sample_name + '.INS.' + key.replace(':', '__') + '.png'
            call, cost, spec = _ins_job((drivers.vapor_simple_ins, num_reads_cff, plt_li, bam_in, ref, ins_pos, ins_seq, fig, '+', phased),
                                        job_cost('INS', len(ins_seq)), ('INS', x[0], x[1], None, ins_seq), mode, key)
            jobs.append(Job(key, call=call, row_prefix=x[3], label=x, cost=cost, spec=spec, ctx=ctx))
            continue
        elif tag in ['a/aa', 'aa/a', 'aa/aa', 'DUP', 'TANDUP']:
            name = 'TANDUP'
        else:
            print(x)
            continue
        key = ':'.join([str(i) for i in x[:-3]] + [name])
        plt_li += 1
        fig = out_path + sample_name + '.' + name + '.' + key.replace(':', '__') + '.png'
        jobs.append(_simple_job(name, x[:-3], key, fig, x[3], x, plt_li, ctx, mode))
    return jobs


def vcf_ci_readin(file_in) -> dict:
    """{'chrom:start:end:TYPE': ((CIPOS lo, hi) or None, (CIEND lo, hi) or None)} of the DEL and INV records of a VCF, the first
    record of a key deciding (as vcf_list_readin keeps the first): the bounds `--refine` keeps a record's candidates within."""
    out = {}
    with open(file_in) as fin:
        for line in fin:
            pin = line.strip().split()
            if not pin or pin[0][0] == '#' or len(pin) < 8:
                continue
            pin[7] = pin[7].replace('MERGE_TYPE=', 'SVTYPE=')
            t = SF.svtype_extract(pin)
            name = 'DEL' if t in ['del', 'DEL', 'deletion'] else 'INV' if t in ['inv', 'INV', 'inversion'] else None
            if name is None:
                continue
            ci = {}
            for x in pin[7].split(';'):
                if x[:6] in ('CIPOS=', 'CIEND='):
                    try:
                        lo, hi = [int(v) for v in x[6:].split(',')]
                    except ValueError:
                        continue
                    ci[x[:5]] = (min(lo, 0), max(hi, 0))
            out.setdefault(':'.join([str(i) for i in SF.chr_start_end_extract(pin)] + [name]), (ci.get('CIPOS'), ci.get('CIEND')))
    return out


def vcf_jobs(vcf_list, num_reads_cff, bam_in, ref, out_path, sample_name, mode=None) -> List[Job]:
    """The loop of vapor_vali/vapor:387-465 (TANDUP is bucketed but never scored there either), and the breakends of
    `vapor vcf --bnd` (vcf_list_readin's last bucket: drivers.vapor_bnd).  `mode`: as in bed_jobs, for the DEL, INV and INS
    records (`--refine` within a record's CIPOS / CIEND, the mode's `ci_of`) and, under `--both-ends`, the breakends."""
    jobs = []
    plt_li = 0
    ctx = (num_reads_cff, bam_in, ref)
    phased = mode is not None and mode.phased
    for x in list(vcf_list.keys()):
        if x not in ('DEL', 'INV', 'INS', 'DISDUP', 'DEL_INV', 'DUP_INV', 'Other', 'BND'):
            print(x)
            continue
        for y in vcf_list[x]:
            if x != 'BND' and 'NA' in y:          # (a breakend's fields are contig names and bases)
                continue
            print(y)
            plt_li += 1
            if x == 'BND':
                key = bnd_key(y)
                fig = out_path + sample_name + '.BND.' + key.replace(':', '__') + '.png'
                if mode is modes.BOTH_ENDS:
                    jobs.append(Job(key, call=(drivers.vapor_both_ends, 'BND', num_reads_cff, plt_li, bam_in, ref, y, fig),
                                    cost=job_cost('BND', 0, views=2)))
                    continue
                jobs.append(Job(key, call=(drivers.vapor_bnd, num_reads_cff, plt_li, bam_in, ref, y, fig), cost=job_cost('BND', 0),
                                bnd=(y, ctx)))
            elif x in ('DEL', 'INV'):
                if y[2] - y[1] < 50:        # both branches label the row DEL (vapor_vali/vapor:394, 407)
                    jobs.append(Job(':'.join([str(i) for i in y] + ['DEL']), fixed=[]))
                    continue
                key = ':'.join([str(i) for i in y] + [x])
                fig = out_path + sample_name + '.' + x + '.' + key.replace(':', '__') + '.png'
                jobs.append(_simple_job(x, y, key, fig, None, None, plt_li, ctx, mode, len(y) == 3))
            elif x == 'INS':
                key = ':'.join([str(i) for i in y[:3] + ['INS']])
                ins_pos = '_'.join([str(i) for i in y[:2]])
                ins_seq = y[-1] if len(y) == 4 else ''.join(['X' for _ in range(y[2])])
                fig = out_path + sample_name + '.INS.' + key.replace(':', '__') + '.png'
                call, cost, spec = _ins_job((drivers.vapor_simple_ins, num_reads_cff, plt_li, bam_in, ref, ins_pos, ins_seq, fig, '+', phased),
                                            job_cost('INS', len(ins_seq)), ('INS', y[0], y[1], None, ins_seq), mode, key)
                jobs.append(Job(key, call=call, cost=cost, spec=spec, ctx=ctx))
            elif x == 'DISDUP':
                key = ':'.join([str(i) for i in y + ['DISDUP']])
                fig = out_path + sample_name + '.DISDUP.' + key.replace(':', '__') + '.png'
                jobs.append(Job(key, call=(drivers.vapor_simple_disdup, num_reads_cff, plt_li, bam_in, ref, y, fig), cost=_dup_cost('DISDUP', y)))
            elif x == 'DEL_INV':
                key = ':'.join(['_'.join([str(i) for i in j]) for j in y] + ['DEL_INV'])
                fig = out_path + sample_name + '.DEL_INV.' + key.replace(':', '__') + '.png'
                jobs.append(Job(key, call=(drivers.vapor_del_inv, num_reads_cff, plt_li, bam_in, ref, y, fig),
                                cost=job_cost('DEL_INV', _num(y[-1][2]) - _num(y[0][1]))))
            elif x == 'DUP_INV':
                key = ':'.join([str(i) for i in y + ['DUP_INV']])
                fig = out_path + sample_name + '.DUP_INV.' + key.replace(':', '__') + '.png'
                jobs.append(Job(key, call=(drivers.vapor_dup_inv, num_reads_cff, plt_li, bam_in, ref, y, fig), cost=_dup_cost('DUP_INV', y)))
            elif x == 'Other':
                key = ':'.join([str(i) for i in y + ['CANNOT_CLASSIFY']])
                fig = out_path + sample_name + '.CANNOT_CLASSIFY.' + key.replace(':', '__') + '.png'
                jobs.append(Job(key, call=(drivers.vapor_cannot_classify, num_reads_cff, plt_li, bam_in, ref, y, fig), cost=_other_cost(y)))
    return jobs


def _num(v) -> int:
    try:
        return int(v)
    except (TypeError, ValueError):
        return 0


def _dup_cost(svtype, y) -> float:
    """DISDUP / DUP_INV record [chrom, s, e, ins_chrom, ins_pos]: the region the drivers cut when block and insert point
    share a contig, the block itself otherwise."""
    s0, e0 = _num(y[1]), _num(y[2])
    if len(y) > 4 and y[0] == y[3]:
        bp = sorted([s0, e0, _num(y[4])])
        return job_cost(svtype, bp[-1] - bp[0], e0 - s0)
    return job_cost(svtype, e0 - s0)


def _other_cost(info) -> float:
    """`Other=` / SVelter record [ref structure, alt structure, chrom, bp, bp, ...]: the span of its numeric fields, once per
    alt allele."""
    nums = [int(v) for v in info[2:] if str(v).isdigit()]
    span = (max(nums) - min(nums)) if len(nums) >= 2 else 0
    n_alt = max(1, len([a for a in str(info[1]).split('_') if a and a not in str(info[0]).split('_')]))
    return n_alt * job_cost('Other', span)


def svelter_readin(file_in):
    """vapor_vali/vapor:255-268: {ref structure: {alt structure: [[chrom, bp, bp, ...], ...]}}."""
    out = {}
    seen = {}                       # (the reference scans the list of a structure pair per record; a set of its entries beside it)
    with open(file_in) as fin:
        fin.readline()
        for line in fin:
            pin = line.strip().split()
            r = '_'.join(pin[4].split('/'))
            a = '_'.join(pin[5].split('/'))
            lst = out.setdefault(r, {}).setdefault(a, [])
            ks = seen.setdefault((r, a), set())
            item = pin[3].split(':')
            if tuple(item) not in ks:
                ks.add(tuple(item))
                lst.append(item)
    return out


def svelter_jobs(sv_hash, num_reads_cff, bam_in, ref, out_path, sample_name) -> List[Job]:
    """The loop of vapor_vali/vapor:481-492."""
    jobs = []
    plt_li = 0
    for k1 in list(sv_hash.keys()):
        for k2 in list(sv_hash[k1].keys()):
            for k3 in sv_hash[k1][k2]:
                plt_li += 1
                key = '.' + '_'.join(k3)
                fig = out_path + sample_name + key.replace(':', '__') + '.png'
                info = [k1, k2] + k3
                print(info)
                jobs.append(Job(key, call=(drivers.vapor_cannot_classify, num_reads_cff, plt_li, bam_in, ref, info, fig), cost=_other_cost(info)))
    return jobs


def output_row(head: list, scores) -> tuple:
    """The line write_output_main (SF:2084-2088) appends for one locus - `head` fields, then what result_organize_ins
    (SF:1219-1231) and gt_estimate_log_likelihood (SF:2054-2069) make of the scores - and the five values behind it
    (finish.row_tail: one rounding per score instead of round -> str -> split -> float).  The reference's test for an
    unscored locus is `'NA' in out_list`, over ALL fields: a head field that reads NA turns GT, GQ and Rec into NA as well."""
    tail = row_tail(scores)
    if tail[0] != 'NA' and 'NA' in head:
        tail = [tail[0], tail[1], 'NA', 'NA', 'NA']
    return '\t'.join([str(i) for i in head + tail]), tail


def output_rows(heads: list, scores_list: list) -> tuple:
    """output_row's line for every locus of the table, and the five values of finish.row_tail behind each (as computed: the
    NA rule of the writer changes the line only - vapor_vali/vapor:357 prints the result before the writer looks at it);
    the tails through finish.row_tails, one call of the library's host helper for the whole table."""
    from .finish import row_tails
    tails = row_tails(scores_list)
    lines = []
    for head, tail in zip(heads, tails):
        if tail[0] != 'NA' and 'NA' in head:
            tail = [tail[0], tail[1], 'NA', 'NA', 'NA']
        lines.append('\t'.join([str(i) for i in head + tail]))
    return lines, tails


def score_jobs(jobs: List[Job], chunk: int, figure_fn=None, mode=None) -> List[object]:
    """Score every job (sharded over ranks, batched on each GPU); returns per job the list of read
    scores, in job order, identical on every rank.  With a `mode` (vapor_amd.modes) every job's `extra` attribute is set as
    well, on every rank: the payload of a locus that has one (refine.Refined.info of a locus that was refined, phase.Phased.phase
    of one that was phased, drivers.BothEnds.views of one that took its junction branch), None otherwise."""
    import gc
    import time
    t0 = time.perf_counter()
    # The cyclic collector looks at every container alive each time its oldest generation is due, and a run keeps its jobs,
    # generators and read lists alive until the table is written: on an 8 000-locus run a quarter of the time went into
    # three or four such passes of ~50 ms, and the share grows with the run.  The loop makes no reference cycles outside its error
    # paths (reference counting frees the rest), so the thresholds are raised for its duration: young objects are still
    # collected every 200 000 net allocations, the older generations practically never.
    gc_was = gc.get_threshold()
    gc.set_threshold(max(gc_was[0], 200000), max(gc_was[1], 50), max(gc_was[2], 1000))
    try:
        return _score_jobs(jobs, chunk, figure_fn, t0) if mode is None else _score_jobs(jobs, chunk, figure_fn, t0, mode)
    finally:
        gc.set_threshold(*gc_was)


def _chunk_threads_ok() -> bool:
    """Chunks are scored on several threads only with a read backend whose handles are per thread - the rule of
    pipeline._prefetch_threads: the Python BGZF reader (VAPOR_BAM_NATIVE=0) shares one file object and block cache between
    seek() and read(), the samtools hybrid and VAPOR_MEMORY_CHOP=records write one module-level result array."""
    from . import seqio
    be = seqio.get_backend()
    if not getattr(be, "chunk_threads_ok", False) or os.environ.get("VAPOR_BAM_NATIVE", "1") == "0":
        return False
    return os.environ.get("VAPOR_MEMORY_CHOP", "") != "records"


def _both_ends_gens(jobs, rest, gens, engine):
    """`--both-ends` from BAM files: the read windows of a chunk's loci - every view's, the primary ones included
    (drivers.both_ends_windows) - go through the device extraction in one call per anchor kind (seqio.prefetch_views:
    bam_chop_kernel, bam_chop_right_kernel), per BAM file, and the loci's generators are made over the file name that carries
    the kept reads by device address.  A window the device leaves to the host route is read by the host reader when its view
    asks.  Returns (the generators, the device batches to close when the chunk is scored); the generators as they were when
    the backend or the engine has no device reader, or figures need the reads as text."""
    from . import _lib, seqio
    be = seqio.get_backend()
    if (not hasattr(be, "chop_many_device") or not hasattr(engine, "bam_chop_device") or os.environ.get("VAPOR_BAM_DEVICE", "1") == "0"
            or os.environ.get("VAPOR_BAM_NATIVE", "1") == "0"):
        return gens, []
    by_bam = {}
    for k, t in enumerate(rest):
        a = jobs[t].call              # (vapor_both_ends, svtype, num_reads_cff, plt_li, bam, ref, info, figure name)
        if a is not None and a[0] is drivers.vapor_both_ends and be.isfile(a[4]):
            by_bam.setdefault(a[4], []).append(k)
    held = []
    gens = list(gens)
    for bam, ks in by_bam.items():
        windows = [w for k in ks for w in drivers.both_ends_windows(jobs[rest[k]].call[1], jobs[rest[k]].call[6])]
        try:
            pre = seqio.prefetch_views(engine, bam, windows)
        except (NotImplementedError, _lib.VaporHipError):       # (a library without the right-anchored device reader)
            continue
        held += pre.batches
        for k in ks:
            a = jobs[rest[k]].call
            gens[k] = a[0](*a[1:4], pre, *a[5:])
    return gens, held


modes.BOTH_ENDS.chunk_gens = _both_ends_gens          # (the only mode that replaces a chunk's generators)


def _evidence_payloads(module):
    """The chunk hook of an evidence mode - `--depth`, `--signatures`, `--links`, `--support` (4.19 to 4.22) -
    from its rule module's reader surface.  The evidence is not a property of a driver's result but of the chunk: the regions
    of all its loci of module.TYPES (module.locus_regions of Job.spec - an INS is spelled [chrom, pos, length] - and, where
    "BND" is among the types, of a breakend's scored view, Job.bnd), array route and drivers' route alike, every window clipped
    to the backend's contig length, go to the read backend in one call of its module.MANY per BAM file; a per-chromosome
    pattern: per file, merged by module.merge_words, the lengths asked of its first file (a pattern that matches none: length
    0, zero answers).  The hook returns {t: module.Payload}; a locus of another type has none."""
    def hook(jobs, todo, engine):
        from . import seqio
        be = seqio.get_backend()
        by_bam = {}
        for t in todo:
            j = jobs[t]
            if j.bnd is not None:
                if "BND" in module.TYPES:
                    by_bam.setdefault((j.bnd[1][1], j.bnd[1][2]), []).append((t, "BND", list(j.bnd[0])))
            elif j.spec is not None and j.ctx is not None and j.spec[0] in module.TYPES:
                name, chrom, s, e, ins_seq = j.spec[:5]
                by_bam.setdefault((j.ctx[1], j.ctx[2]), []).append((t, name, [chrom, s, len(ins_seq)] if name == 'INS' else [chrom, s, e]))
        out = {}
        for (bam, ref), loci in by_bam.items():
            files = seqio.bam_in_decide(bam, None)

            def length_of(chrom):
                return be.contig_length(files[0], ref, chrom) if files else 0
            where, sent = [], []
            for _t, name, locus in loci:
                regs = module.locus_regions(name, locus, length_of)
                where.append((len(sent), regs))
                sent += regs
            chroms, rows = [c for c, _f, _p in sent], [f for _c, f, _p in sent]
            partners = ([p for _c, _f, p in sent],) if module.LINKED else ()
            got = [list(module.ZERO) for _ in sent]
            for f in files:
                for k, a in enumerate(getattr(be, module.MANY)(engine, f, chroms, rows, *partners)):
                    got[k] = module.merge_words(got[k], a)
            for (t, name, locus), (at, regs) in zip(loci, where):
                out[t] = module.locus_payload(name, locus, regs, got[at:at + len(regs)])
        return out
    return hook


for _mode, _module in ((modes.DEPTH, depth), (modes.SIGNATURES, signature), (modes.LINKS, links), (modes.SUPPORT, support)):
    _mode.chunk_payloads = _evidence_payloads(_module)


last_timing: dict = {}          # of the most recent score_jobs: seconds scoring this rank's share, seconds in the gather


def _score_jobs(jobs, chunk, figure_fn, t0, mode=None):
    import time
    # shares by estimated cost (greedy longest-processing-time), the same list on every rank
    costs = [float(j.cost) for j in jobs]
    mine = vdist.my_share(len(jobs), costs)
    local: dict = {}
    payloads: dict = {}            # of a mode with chunk_payloads: {job: payload}, written by one_chunk (a chunk's jobs are its own)

    def one_chunk(a, engine=None):
        part = mine[a:a + chunk]
        todo = [t for t in part if jobs[t].make is not None]
        done = {}
        if figure_fn is None and os.environ.get("VAPOR_FAST_PATH", "1") != "0":
            # the simple types of the chunk in array form (vapor_amd.fastpath); what leaves the drivers' straight route comes
            # back unanswered and goes the generators' way below - as everything does when figures are drawn (they need the
            # best read as text)
            from . import fastpath, seqio
            by_ctx = {}
            for t in todo:
                j = jobs[t]
                if j.spec is not None and j.ctx is not None:
                    by_ctx.setdefault(j.ctx, []).append(t)
            for ctx, ts in by_ctx.items():
                eng = engine or pipeline.get_engine()
                if len(ts) >= 8 and fastpath.capable(seqio.get_backend(), ctx[1], eng):
                    got = fastpath.run(eng, [jobs[t].spec for t in ts], ctx[1], ctx[2], ctx[0], **({"phased": True} if mode is not None and mode.phased else {}))
                    for t, r in zip(ts, got):
                        if r is not fastpath.FALLBACK:
                            done[t] = r
        rest = [t for t in todo if t not in done]
        gens, held = [jobs[t].make() for t in rest], []
        if mode is not None and mode.chunk_gens is not None and figure_fn is None and rest:
            gens, held = mode.chunk_gens(jobs, rest, gens, engine or pipeline.get_engine())
        try:
            res = pipeline.run_batch(gens, engine=engine, figure_fn=figure_fn) if rest else []
        finally:
            del gens
            for bt in held:                          # (the reads' blocks on the device: the sets made from them are closed)
                bt.close()
        for t, r in zip(rest, res):
            done[t] = r
        if mode is not None and mode.chunk_payloads is not None and todo:
            # (a payload of the chunk, not of a driver's result: one call for all its loci, whichever route scored them)
            payloads.update(mode.chunk_payloads(jobs, todo, engine))
        if mode is not None and mode.sink is not None:
            # (`--realign-out`: the rank that scored a locus writes it, as figures are written; the sink orders by job)
            for t in todo:
                if not isinstance(done[t], BaseException) and done[t] is not None:
                    mode.sink.take(t, jobs[t].key, getattr(done[t], mode.attr, None))
        return part, todo, [done[t] for t in todo]

    in_flight = max(1, int(os.environ.get("VAPOR_CHUNKS_IN_FLIGHT", "3")))
    if in_flight >= 2 and not _chunk_threads_ok():
        in_flight = 1
    if in_flight >= 2 and 256 <= len(mine) <= chunk:
        # a share of one chunk: in halves (thirds from 1 536 loci on), so that every thread has one - the native half of a
        # chunk's work (read selection, upload, planning, kernels) runs beside the others' Python
        chunk = -(-len(mine) // (min(in_flight, 3) if len(mine) >= 1536 else 2))
    starts = list(range(0, len(mine), max(chunk, 1)))
    if len(starts) >= 2 and in_flight >= 2:
        # Two chunks in flight (the reference's loop over loci, vapor_vali/vapor:334-367, has no such stage): each on a thread
        # with a library context of its own (one host thread per context), so that the host preparation of one chunk - allele
        # strings, read extraction, tables - runs while the other waits for its uploads and kernels; on the device the two
        # contexts' streams overlap as well.  Results are taken in chunk order.
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(in_flight, len(starts))) as pool:
            import threading
            slot = {}
            shared = set()
            lock = threading.Lock()

            def work(a):
                with lock:
                    k = slot.setdefault(threading.get_ident(), len(slot))
                eng = pipeline.engine_slot(k)
                if k not in shared and hasattr(eng, "set_param"):
                    # several chunks at once: a chunk's read extraction on the device keeps to five eighths of the CUs, so that
                    # the other chunks' packing / join / clean kernels do not wait behind its inflating wavefronts
                    shared.add(k)
                    try:
                        eng.set_param("bam_cu_share", int(os.environ.get("VAPOR_BAM_CU_EIGHTHS", "5")))
                    except Exception:       # noqa: BLE001 - an engine without the parameter (tests' stand-ins)
                        pass
                return one_chunk(a, eng)
            try:
                done = list(pool.map(work, starts))
            finally:
                for k in shared:                       # (a later run of one chunk has the device to itself)
                    try:
                        pipeline.engine_slot(k).set_param("bam_cu_share", 0)
                    except Exception:       # noqa: BLE001
                        pass
    else:
        done = [one_chunk(a) for a in starts]
    for part, todo, res in done:
        for t, r in zip(todo, res):
            local[t] = r
        for t in part:
            if jobs[t].make is None:
                local[t] = jobs[t].fixed
    t1 = time.perf_counter()
    if mode is not None:
        # (the extra columns travel as a second table of "scores": mode.pack's floats for a locus with a payload, none otherwise)
        if mode.chunk_payloads is not None:
            extra = {t: mode.pack(payloads.get(t)) for t in local}
        else:
            extra = {t: (mode.pack(getattr(r, mode.attr, None)) if not isinstance(r, BaseException) and r is not None else [])
                     for t, r in local.items()}
        for j, v in zip(jobs, vdist.gather_results(extra, len(jobs), costs)):
            j.extra = mode.unpack(v)
    allres = vdist.gather_results(local, len(jobs), costs)
    last_timing.update(score_s=t1 - t0, gather_s=time.perf_counter() - t1, loci=len(mine), cost=sum(costs[t] for t in mine))
    if os.environ.get("VAPOR_TIMING") and vdist.rank() == 0:
        dt = time.perf_counter() - t0
        print("vapor_amd.cli: scored %d loci on %d rank(s) in %.3f s -> %.1f loci/s" % (len(jobs), vdist.world(), dt, len(jobs) / dt),
              file=sys.stderr)
    for r in allres:
        if isinstance(r, BaseException):
            raise r
    return allres


# ------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="vapor", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--sv-input', required=True, help='input file of SV calls')
    p.add_argument('--reference', required=True, help='reference sequences')
    p.add_argument('--pacbio-input', required=True, help='input pacbio sequences in bam format')
    p.add_argument('--output-path', required=True, help='path of output VaPoR figures')
    p.add_argument('--output-file', required=True, help='name of output file')
    p.add_argument('--PB-supp', required=False, help='minimum number of evaluable PacBio reads')
    p.add_argument('--no-figures', action='store_true', help='do not render recurrence-plot PNGs')
    p.add_argument('--chunk', type=int, default=2048, help='loci per device batch')
    p.add_argument('--bnd', action='store_true',
                   help='vcf: also score breakend (SVTYPE=BND) records: t[B:q[, t]B:q] and ]B:q]t junctions')
    p.add_argument('--refine', metavar='M[:T]', default=None,
                   help='bed, vcf: score candidate breakpoints within M bp of every short DEL / INV / TANDUP call, in steps of T bp '
                        '(default: the smallest step that keeps a locus within 128 candidates), and report the best; appends '
                        'VaPoR_RPOS, VaPoR_REND, VaPoR_QS0 and VaPoR_GS0 (vcf: to INFO, within CIPOS / CIEND)')
    p.add_argument('--phased', action='store_true',
                   help='bed, vcf: read the HP and PS tags of a haplotagged BAM; every DEL / INV / TANDUP / INS call is scored per '
                        'haplotype as well (the reads with HP 1, with HP 2, of the majority phase set): appends VaPoR_PS, VaPoR_PGT, '
                        'VaPoR_PGQ and VaPoR_H1_QS / _GS / _Rec, VaPoR_H2_QS / _GS / _Rec (vcf: to INFO); not together with --refine')
    p.add_argument('--phase-vcf', metavar='FILE', default=None,
                   help='bed, vcf: --phased for a BAM that is not haplotagged: FILE is a phased small-variant VCF of the sample (plain '
                        'or gzipped); a read is assigned the haplotype most of its bases at the phased heterozygous SNVs within '
                        '100 kb of the locus vote for, in the phase set with the most votes; the HP / PS tags of the BAM are not read')
    p.add_argument('--phase-sample', metavar='NAME', default=None,
                   help='with --phase-vcf: the sample column of FILE to read (default: the first)')
    p.add_argument('--both-ends', action='store_true',
                   help='bed, vcf: score every junction - a DEL or INV of 10 kb or more, the junction branch of a TANDUP, every '
                        'breakend of --bnd - from both of its sides: the reads that end behind the window (right-anchored) are scored '
                        'as well, [B:q[t breakends are taken; appends VaPoR_BE_N, VaPoR_BE_QS / _GS / _GT / _GQ / _Rec and VaPoR_BE_SQS '
                        '(vcf: to INFO); not together with --refine or --phased')
    p.add_argument('--depth', action='store_true',
                   help='bed, vcf: compare read depth inside every DEL and TANDUP call with the depth of its 1 kb flanks (an event '
                        'above 20 kb: 10 kb at each of its ends); unmapped, secondary, QC-fail and duplicate records never count; '
                        'appends VaPoR_DP_IN, VaPoR_DP_FL, VaPoR_DFC and VaPoR_DSUP - 1 where the fold change is below 0.7 for a DEL, '
                        'above 1.3 for a TANDUP (vcf: to INFO); not together with --refine, --phased, --phase-vcf or --both-ends')
    p.add_argument('--signatures', action='store_true',
                   help='bed, vcf: split-read and CIGAR evidence per DEL, TANDUP, INV and INS call: alignments soft- or hard-clipped by '
                        '30 bases or more within 50 bases of a breakpoint, alignments that carry the event as a D or N (DEL) or an I '
                        '(INS, TANDUP) of a fitting length, and the modal breakpoints they give; unmapped, secondary, QC-fail and '
                        'duplicate records never count, supplementary records do; appends VaPoR_SIG_L, VaPoR_SIG_R, VaPoR_SIG_CG, '
                        'VaPoR_SIG_N, VaPoR_SIG_POS and VaPoR_SIG_END (vcf: to INFO); not together with --refine, --phased, '
                        '--phase-vcf, --both-ends or --depth')
    p.add_argument('--links', action='store_true',
                   help='bed, vcf: split reads joined through their SA tags, per DEL, TANDUP and INV call and per breakend of --bnd: '
                        'alignments soft- or hard-clipped by 30 bases or more within 50 bases of a breakpoint whose SA tag names a piece '
                        'within 50 bases of the other breakpoint, on the strand the event gives it; clipped alignments whose SA '
                        'entries all lie elsewhere; and the modal coordinates the linked pieces name; unmapped, secondary, QC-fail and '
                        'duplicate records never count, supplementary records do, --min-mapq holds for the entries as well; appends '
                        'VaPoR_LNK_L, VaPoR_LNK_R, VaPoR_LNK_N, VaPoR_LNK_OL, VaPoR_LNK_OR, VaPoR_LNK_POS and VaPoR_LNK_END (vcf: to '
                        'INFO); not together with --refine, --phased, --phase-vcf, --both-ends, --depth or --signatures')
    p.add_argument('--support', action='store_true',
                   help='bed, vcf: alt and ref alignments per DEL, TANDUP, INV and INS call: the records that carry the event as '
                        '--signatures counts them (once a record), the records that reach 51 bases to either side of a breakpoint '
                        'with no D, N or I of 30 bases or more near it, and the records that cover each breakpoint; unmapped, '
                        'secondary, QC-fail and duplicate records never count, supplementary records do; appends VaPoR_SUP_ALT, '
                        'VaPoR_SUP_REF, VaPoR_SUP_REFL, VaPoR_SUP_REFR, VaPoR_SUP_COVL, VaPoR_SUP_COVR, VaPoR_SUP_VAF, VaPoR_SUP_GT and '
                        'VaPoR_SUP_GQ (vcf: to INFO; no VAF, GT or GQ for a TANDUP); not together with --refine, --phased, '
                        '--phase-vcf, --both-ends, --depth, --signatures or --links')
    # (`--realign`, DESIGN.md 4.23: every read aligned to both alleles on the device, VaPoR_RA_* behind the row.  Its paragraph is
    # README.md's until the recording of this help text is made again: SUPPRESS keeps the option out of the usage line and the list)
    p.add_argument('--realign', action='store_true', help=argparse.SUPPRESS)
    # (`--realign-out PREFIX`, DESIGN.md 4.24: every read's alignment to the allele it fits, PREFIX.sam over PREFIX.fa; no mode
    # of its own - it needs --realign - and suppressed for the same reason)
    p.add_argument('--realign-out', metavar='PREFIX', default=None, help=argparse.SUPPRESS)
    # (`--realign-polish`, DESIGN.md 4.25: the ALT voters piled on the alt allele, six columns behind --realign's and, with
    # --realign-out, PREFIX.pol.fa; no mode of its own - it needs --realign - and suppressed for the same reason)
    p.add_argument('--realign-polish', action='store_true', help=argparse.SUPPRESS)
    # (`--realign-junction`, DESIGN.md 4.26: the polished allele read as one jump of its window, six columns behind
    # --realign-polish's; no mode of its own - it needs --realign-polish - and suppressed for the same reason)
    p.add_argument('--realign-junction', action='store_true', help=argparse.SUPPRESS)
    # (`--realign-revote`, DESIGN.md 4.27: every read aligned once more, against the polished allele, eight columns behind
    # everything else the run appends; no mode of its own - it needs --realign-polish - and suppressed for the same reason)
    p.add_argument('--realign-revote', action='store_true', help=argparse.SUPPRESS)
    p.add_argument('--min-mapq', metavar='Q', type=_int_in('--min-mapq', 0, 255), default=0,
                   help='every sub-command: skip records with MAPQ below Q (0..255, default 0), as `samtools view -q Q` does; a '
                        'filtered record is treated as if it were not in the file')
    p.add_argument('--exclude-flags', metavar='F', type=_int_in('--exclude-flags', 0, 65535), default=0,
                   help='every sub-command: skip records with any bit of F set in FLAG (0..65535, decimal or 0x hex, default 0), as '
                        '`samtools view -F F` does; for minimap2 / pbmm2 files --min-mapq 20 --exclude-flags 0x704 (unmapped, '
                        'secondary, QC-fail, duplicate) is a sensible start, and 0x800 (supplementary) is the user\'s choice')
    p.add_argument('--dedup-qname', action='store_true',
                   help='every sub-command: records with one QNAME are one molecule - of the kept records of a region one per QNAME '
                        'survives (the first that is neither secondary nor supplementary, else the first); with --both-ends a '
                        'molecule that is kept in several views counts once in the pooled VaPoR_BE_* columns')
    return p


def _int_in(name, lo, hi):
    """argparse type: an integer in lo..hi as int(x, 0) reads it (decimal or 0x hex); anything else is a parser error."""
    def parse(text):
        try:
            v = int(text, 0)
        except (TypeError, ValueError):
            raise argparse.ArgumentTypeError('%s takes an integer (decimal or 0x hex), not %r' % (name, text)) from None
        if not lo <= v <= hi:
            raise argparse.ArgumentTypeError('%s must be between %d and %d, not %r' % (name, lo, hi, text))
        return v
    return parse


# "A run has one mode" (vapor_amd/modes.py), as the parser says it: the options that make a mode, in the order their refusals are
# checked, and what a pair is told where that is more than the rule.  `--phase-vcf` is `--phased` with another source of tags:
# the three older modes refuse it under that name (None: not under its own).
MODE_OPTIONS = ('--refine', '--phase-vcf', '--phased', '--both-ends', '--depth', '--signatures', '--links', '--support', '--realign')
PAIR_REASONS = {
    ('--phased', '--refine'): 'refinement per haplotype is not implemented',
    ('--phased', '--phase-vcf'): None,
    ('--both-ends', '--refine'): 'refined candidates are scored from one side',
    ('--both-ends', '--phase-vcf'): None,
    ('--both-ends', '--phased'): 'right-anchored reads are not read with their tags',
    ('--depth', '--refine'): 'depth is measured over the called breakpoints',
    ('--depth', '--phase-vcf'): 'depth is not measured per haplotype',
    ('--depth', '--phased'): 'depth is not measured per haplotype',
    ('--signatures', '--phase-vcf'): 'signatures are not counted per haplotype',
    ('--signatures', '--phased'): 'signatures are not counted per haplotype',
    ('--links', '--phase-vcf'): 'links are not counted per haplotype',
    ('--links', '--phased'): 'links are not counted per haplotype',
}


def main(argv: Optional[List[str]] = None) -> int:
    held: list = []                      # (`--phase-vcf`, the read filter: the backend that carries the run's sites and its (Q, F), for as long as the run lasts)
    try:
        return _main(argv, held)
    finally:
        for backend in held:
            backend.phase_sites = None
            backend.read_filter = (0, 0)
            backend.dedup_qname = False


def _write_table(path, heads, jobs, scores, mode) -> list:
    """A table: the header, a row per job (result_organize_ins + write_output_main of vapor_vali/vapor:356-357 in one go:
    finish.row_tails) with the mode's columns behind it.  Returns the rows' tails (output_rows)."""
    SF.write_output_initiate(path, mode.COLUMNS if mode is not None else ())
    lines, tails = output_rows(heads, scores)
    if mode is not None:
        lines = [l + '\t' + '\t'.join(c) for l, c in zip(lines, mode.columns_many([j.extra for j in jobs]))]
    with open(path, 'a') as fo:
        fo.write(''.join([l + '\n' for l in lines]))
    return tails


def _main(argv, held) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    if len(argv) < 1:
        from . import prep
        prep.print_read_me()
        return 0
    cmd = argv[0]
    if len(argv) == 1:
        from . import prep
        {'bed': prep.readme_bed, 'vcf': prep.readme_vcf, 'ins': prep.readme_melt}.get(cmd, prep.print_read_me)()
        return 0
    parser = build_parser()
    args = parser.parse_args(argv[1:])
    num_reads_cff = int(args.PB_supp) if args.PB_supp else 3
    refine = None
    if args.refine is not None:
        from . import refine as rf
        if cmd not in ('bed', 'vcf'):
            parser.error('--refine applies to `vapor bed` and `vapor vcf`')
        try:
            refine = rf.parse(args.refine)
        except ValueError as e:
            parser.error(str(e))
    if args.phase_sample is not None and args.phase_vcf is None:
        parser.error('--phase-sample names a sample of --phase-vcf: give that option too')
    if args.realign_out is not None and not args.realign:
        parser.error('--realign-out needs --realign')
    if args.realign_polish and not args.realign:
        parser.error('--realign-polish needs --realign')
    if args.realign_junction and not args.realign_polish:
        parser.error('--realign-junction needs --realign-polish')
    if args.realign_revote and not args.realign_polish:
        parser.error('--realign-revote needs --realign-polish')
    if args.phase_vcf is not None:
        args.phased = True               # (the groups, the scoring and the columns are --phased's: only the tags' source differs)
    # a run has one mode: every later option of MODE_OPTIONS refuses the sub-commands it does not apply to, then each earlier one
    given = dict(zip(MODE_OPTIONS, (refine is not None, args.phase_vcf is not None, args.phased, args.both_ends, args.depth, args.signatures,
                                    args.links, args.support, args.realign)))
    for k, opt in enumerate(MODE_OPTIONS[2:], 2):           # (--refine's block stands above, --phase-vcf is --phased here)
        if not given[opt]:
            continue
        if cmd not in ('bed', 'vcf'):
            parser.error('%s applies to `vapor bed` and `vapor vcf`' % opt)
        for other in MODE_OPTIONS[:k]:
            why = PAIR_REASONS.get((opt, other), 'a run has one mode')
            if given[other] and why is not None:
                parser.error('%s and %s cannot be combined (%s)' % (opt, other, why))
    if args.phase_vcf is not None:
        # (every rank reads the VCF itself; the sites ride on the backend the reads are taken through)
        from . import phase as ph
        try:
            sites = ph.read_sites(args.phase_vcf, args.phase_sample)
        except (OSError, ValueError) as e:
            parser.error('--phase-vcf: %s' % e)
        from . import seqio
        backend = seqio.get_backend()
        backend.phase_sites = sites
        held.append(backend)
    if args.min_mapq or args.exclude_flags:
        # (set once, on the backend every read route takes its records through)
        from . import seqio
        backend = seqio.get_backend()
        backend.read_filter = (args.min_mapq, args.exclude_flags)
        if backend not in held:
            held.append(backend)
    if args.dedup_qname:
        # (likewise - rule W where the records are kept, rule V where the views are pooled)
        from . import seqio
        backend = seqio.get_backend()
        backend.dedup_qname = True
        if backend not in held:
            held.append(backend)
    mode = None                          # (at most one mode: every pair of the options that make one was refused above)
    if refine is not None:
        mode = modes.refine(*refine, ci_of=vcf_ci_readin(args.sv_input) if cmd == 'vcf' else None)
    elif args.phased:
        mode = modes.PHASED
    elif args.both_ends:
        mode = modes.BOTH_ENDS
    elif args.depth:
        mode = modes.DEPTH
    elif args.signatures:
        mode = modes.SIGNATURES
    elif args.links:
        mode = modes.LINKS
    elif args.support:
        mode = modes.SUPPORT
    figure_fn = None
    if not args.no_figures:
        from . import figures
        figure_fn = figures.make_event_figure_1
        figures.warm()                  # (the drawing processes start while the input is parsed and the first batch scored)
    vdist.init_from_env()
    if args.realign:
        # (what the run asks beside the votes, and with `--realign-out` the sink of the rank's traces)
        from . import polish, realign
        options = realign.Options(args.realign_out is not None, args.realign_polish, args.realign_junction, args.realign_revote)
        writer = polish.PolishWriter if options.polish else realign.TraceWriter
        mode = modes.realign(options, writer(args.realign_out, vdist.rank(), vdist.world()) if options.trace else None)
    out_path = SF.path_modify(args.output_path)
    SF.path_mkdir(out_path)
    sample_name = '.'.join(args.sv_input.split('/')[-1].split('.')[:-1])
    bam_in, ref = args.pacbio_input, args.reference
    if cmd == 'bed':
        bed_info = bed_info_readin(args.sv_input, out_path)
        jobs = bed_jobs(bed_info, num_reads_cff, bam_in, ref, out_path, sample_name, mode)
        scores = score_jobs(jobs, args.chunk, figure_fn, mode)
        if vdist.rank() == 0:
            tails = _write_table(args.output_file, [j.key.split(':') + [j.row_prefix] for j in jobs], jobs, scores, mode)
            for j, tail in zip(jobs, tails):
                print([j.key, tail[0], tail[1], tail[4]])
    elif cmd == 'vcf':
        vcf_list, rec_hash = vcf_list_readin(args.sv_input, ref if args.bnd else None, args.both_ends)
        rec_new = SF.vcf_rec_hash_modify(rec_hash)
        jobs = vcf_jobs(vcf_list, num_reads_cff, bam_in, ref, out_path, sample_name, mode)
        scores = score_jobs(jobs, args.chunk, figure_fn, mode)
        if vdist.rank() == 0:
            _write_table(args.sv_input + '.vapor', [[j.key] for j in jobs], jobs, scores, mode)
            SF.vcf_vapor_modify(args.sv_input, rec_new, mode=mode)
    elif cmd == 'svelter':
        jobs = svelter_jobs(svelter_readin(args.sv_input), num_reads_cff, bam_in, ref, out_path, sample_name)
        scores = score_jobs(jobs, args.chunk, figure_fn)
        if vdist.rank() == 0:
            with open(args.output_file, 'a') as fo:      # appended, never initialised (vapor_vali/vapor:492)
                fo.write(''.join([l + '\n' for l in output_rows([[j.key] for j in jobs], scores)[0]]))
    elif cmd == 'ins':
        from . import melt
        melt.run(args.sv_input, out_path, sample_name.split('.')[0], bam_in, ref, num_reads_cff, args.chunk, figure_fn)
    else:
        raise SystemExit("vapor: unknown mode %r (bed | vcf | svelter | ins)" % cmd)
    if mode is not None and mode.sink is not None:
        mode.sink.close()
    vdist.finalize()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

"""`vapor bed | vcf --support` without a GPU: the parser, the regions of a locus (support.regions), a region's
seven words (support.answer) against a brute-force statement written here - every record expanded to one operation code per
reference position, its class read off that map - the disjointness of the classes, the genotype of two counts, the mode's
surface, the native host reader (vapor_bam_support) against both on files written case by case, tools/bam_check.cpp's sup pass
and tools/readplan_check.cpp under the sanitizers as programs of their own, and cli.main on a world whose nine columns are known
in closed form (synth.make_support_world).  Device work of the row's own columns is answered by tests/fake_engine.py
(oracle-backed, test only).  Every comparison is on integers and exact."""
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import readplan_program
import test_bamio as TB
import test_modes_cpu as TM
import test_signature_cpu as TS
from fake_engine import FakeEngine
from vapor_amd import _lib as L
from vapor_amd import bamio, cli, modes, pipeline, seqio, signature, support, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = TS.BASE
C, T, P, F, G = 30, 50, 10000, 51, 30
NCAP = (1 << 28) - 1
LC0, RC0, LC1, RC1, GAP, INSOP, REF0, REF1 = 1, 2, 4, 8, 16, 32, 64, 128
M, I, D, N, S, H, PAD, EQ, X = range(9)


# ------------------------------------------------------------------------------------------------------------------------------
# the parser
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_parser_takes_support_on_bed_and_vcf():
    assert cli.build_parser().parse_args(BASE).support is False
    assert cli.build_parser().parse_args(BASE + ["--support"]).support is True
    assert cli.build_parser().parse_args(BASE + ["--support", "--min-mapq", "20", "--exclude-flags", "0x800", "--dedup-qname", "--bnd",
                                                 "--no-figures"]).support is True
    m = modes.SUPPORT
    assert m.name == "support" and m.chunk_payloads is not None and m.chunk_gens is None
    assert tuple(TM.hook_payloads(m)) == support.TYPES          # the hook answers for the module's types
    assert (support.F, support.G, support.T, support.C, support.P, support.EXCLUDE, support.ERR) == (F, G, T, C, P, 0x704, 0.05)
    assert support.FIELDS == signature.FIELDS + ("flank", "gmin") and len(support.FIELDS) == 11 and len(support.WORDS) == 7
    assert support.TYPES == signature.TYPES == ("DEL", "TANDUP", "INV", "INS") and (support.REF0, support.REF1) == (REF0, REF1)


@pytest.mark.parametrize("cmd, more, message", [
    ("bed", ["--support", "--refine", "20"], "--support and --refine cannot be combined (a run has one mode)"),
    ("vcf", ["--support", "--phased"], "--support and --phased cannot be combined (a run has one mode)"),
    ("bed", ["--support", "--phase-vcf", "p.vcf"], "--support and --phase-vcf cannot be combined (a run has one mode)"),
    ("vcf", ["--support", "--both-ends"], "--support and --both-ends cannot be combined (a run has one mode)"),
    ("bed", ["--support", "--depth"], "--support and --depth cannot be combined (a run has one mode)"),
    ("bed", ["--support", "--signatures"], "--support and --signatures cannot be combined (a run has one mode)"),
    ("vcf", ["--support", "--links"], "--support and --links cannot be combined (a run has one mode)"),
    ("svelter", ["--support"], "--support applies to `vapor bed` and `vapor vcf`"),
    ("ins", ["--support"], "--support applies to `vapor bed` and `vapor vcf`"),
])
def test_refused_option_combinations(cmd, more, message, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main([cmd] + BASE + more)
    assert e.value.code == 2 and message in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------------------------------------
# support.regions
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("svtype", ["DEL", "TANDUP", "INV"])
def test_regions_at_the_split_threshold(svtype):
    n = 10 ** 6
    s = 50000
    mask = TS.MASKS[svtype]
    e = s - 1 + P                                 # J1 - J0 = P: one region, both bits
    nmin, nmax = (max(30, (P + 1) // 2), 2 * P) if svtype != "INV" else (0, 0)
    assert support.regions(svtype, ["c", s, e], n) == [(s - 1 - F, e + F, s - 1, e, T, C, nmin, nmax, mask | REF0 | REF1, F, G)]
    e += 1                                        # P + 1: two regions, bit 6 in each, the second's targets both J1
    first, second = support.regions(svtype, ["c", s, e], n)
    gap = svtype == "DEL"
    length = P + 1
    assert first == (s - 1 - F, s - 1 + F, s - 1, e, T, C, max(30, (length + 1) // 2) if gap else 0, 2 * length if gap else 0,
                     mask & (LC0 | RC0 | GAP) | REF0, F, G)
    assert second == (e - F, e + F, e, e, T, C, 0, 0, (mask >> 2) & 3 | REF0, F, G)
    # the first nine fields are signature.regions', the windows among them
    for loc in (["c", s, s - 1 + P], ["c", s, e]):
        assert [r[:8] + (r[8] & 63,) for r in support.regions(svtype, loc, n)] == signature.regions(svtype, loc, n)


def test_regions_of_an_insertion_at_both_contig_ends_with_one_base_and_of_other_types():
    n = 10 ** 6
    for length in (P, P + 1, 5 * P):
        assert support.regions("INS", ("c", 7000, length), n) == [(7000 - F, 7000 + F, 7000, 7000, T, C, max(30, (length + 1) // 2), 2 * length,
                                                                   TS.MASKS["INS"] | REF0 | REF1, F, G)]
    for t in ("BND", "DISDUP", "DEL_INV", "DUP_INV", "Other"):
        assert support.regions(t, ["c", 500, 900], n) == []
    # the left end: x - F < 0, the window starts at 0; the right end: the window ends with the contig; a contig the file lacks
    assert support.regions("DEL", ["c", 10, 400], 5000)[0][:4] == (0, 400 + F, 9, 400)
    assert support.regions("INV", ["c", 4000, 4990], 5000)[0][:4] == (3999 - F, 5000, 3999, 4990)
    assert support.regions("DEL", ["c", 4000, 4500], 0)[0][:2] == (0, 0)
    assert support.regions("INS", ("c", 0, 100), 5000)[0][:4] == (0, F, 0, 0)
    far = support.regions("DEL", ["c", 100, 100 + 3 * P], 2 * P)
    assert [r[:2] for r in far] == [(99 - F, 99 + F), (2 * P, 2 * P)] and [r[8] & (REF0 | REF1) for r in far] == [REF0, REF0]
    # L = 1: no operation can count, the CIGAR bit is off; reference support is still asked
    for t in ("DEL", "TANDUP", "INS"):
        r = support.regions(t, ["c", 700, 700] if t != "INS" else ("c", 700, 1), 5000)
        assert len(r) == 1 and r[0][6:] == (0, 0, TS.MASKS[t] & 15 | REF0 | REF1, F, G)
    for t in TS.MASKS:
        for loc in (["c", 2, 30000], ["c", 700, 900], ["c", 4990, 5100]):
            for r in support.regions(t, loc, 5000):
                # tol < F and g <= nmin wherever a CIGAR bit is on: what the exclusion argument of 4.22 needs
                assert support.region_ok(r) and r[4] < r[9] and (not r[8] & (GAP | INSOP) or r[10] <= r[6])


# ------------------------------------------------------------------------------------------------------------------------------
# support.answer against a brute-force statement
# ------------------------------------------------------------------------------------------------------------------------------
def brute_one(pos0, ops, region):
    """The model: the record as one operation code per reference position (and the run it belongs to), its insertions at the
    boundaries between positions, its clips counted off the expansion - and the record's class read off that map.  Returns the
    record's seven words."""
    _w0, _w3, x0, x1, tol, min_clip, nmin, nmax, mask, flank, gmin = region
    x = [code for n, code in ops for _ in range(n)]
    if not x or all(c in (S, H) for c in x):
        return [0] * 7
    lead = next(i for i, c in enumerate(x) if c not in (S, H))
    trail = next(i for i, c in enumerate(reversed(x)) if c not in (S, H))
    ref = {}                       # reference position -> (code, length of its run)
    ins = []                       # (boundary before reference position a, length)
    cur = pos0
    for n, code in ops:
        if code in (M, D, N, EQ, X):
            for p in range(cur, cur + n):
                ref[p] = (code, n, cur)
            cur += n
        elif code == I:
            ins.append((cur, n))
    q = cur
    assert q == pos0 + len(ref)
    need = max(min_clip, 1)
    xs = (x0, x1)
    runs = {(a, n) for code, n, a in ref.values() if code in (D, N)}
    cg = (bool(mask & GAP) and any(nmin <= n <= nmax and abs(a - x0) <= tol and abs(a + n - x1) <= tol for a, n in runs)) or \
         (bool(mask & INSOP) and any(nmin <= n <= nmax and x0 - tol <= a <= x1 + tol for a, n in ins))
    out = [int(cg), 0, 0, 0, 0, 0, 0]
    for k in (0, 1):
        clip = (mask >> (2 * k) & 1 and lead >= need and abs(pos0 - xs[k]) <= tol) or (mask >> (2 * k + 1) & 1 and trail >= need and abs(q - xs[k]) <= tol)
        # a spanner: every reference position of [x - F, x + F) is the record's, none in a D or N of gmin bases, and no I of gmin
        # bases at a boundary from x - F to x + F
        span = all(p in ref and not (ref[p][0] in (D, N) and ref[p][1] >= gmin) for p in range(xs[k] - flank, xs[k] + flank)) and \
            not any(n >= gmin and xs[k] - flank <= a <= xs[k] + flank for a, n in ins)
        out[1 + k] = int(bool(clip) and not cg)
        out[3 + k] = int(bool(mask & (REF0, REF1)[k]) and span and not cg and not clip)
        out[5 + k] = int(xs[k] in ref)
    return out


def brute(records, region, min_mapq=0, exclude=0):
    """A region's seven words.  records: (pos0, [(n, code)...], mapq, flag)."""
    out = [0] * 7
    for pos0, ops, mapq, flag in records:
        if mapq < min_mapq or flag & (exclude | 0x704) or pos0 >= region[1] or region[1] <= region[0]:
            continue
        out = [a + b for a, b in zip(out, brute_one(pos0, ops, region))]
    return out


def statement(records, region, min_mapq=0, exclude=0):
    kept = [r for r in records if not (r[2] < min_mapq or r[3] & (exclude | 0x704))]
    return support.answer(TS.as_records(kept), region)


ALL = 255
REGIONS = [
    (1900, 3200, 2000, 3000, 50, 30, 1, 500, ALL, F, G),
    (1900, 2200, 2050, 2050, 50, 30, 1, NCAP, ALL, F, G),              # x0 == x1
    (0, 9000, 2500, 2600, 255, 1, 0, NCAP, ALL, 20, 1),                # tol far above F: clips and spanners meet
    (2400, 2700, 2500, 2600, 0, 10, 0, NCAP, ALL, 1, 1),               # the narrowest flank
    (1900, 3200, 2000, 3000, 50, 30, 40, 80, GAP | INSOP | REF0 | REF1, 100, 60),
    (1900, 3200, 2000, 3000, 50, 30, 0, 0, 15, F, G),                  # bits 6 and 7 off
    (1900, 3200, 2000, 3000, 50, 30, 1, 500, REF1, 300, NCAP + 1),     # nothing blocks, one bit
    (2500, 2500, 2450, 2450, 40, 30, 1, 500, ALL, F, G),               # an empty window
    (0, 2051, 30, 2000, 50, 30, 1, NCAP, RC0 | GAP | REF0, F, G),      # x0 - F < 0
    (1949, 2051, 2000, 6000, 50, 30, 1, NCAP, RC0 | GAP | REF0, F, G),     # the first region of a long event
]


def test_answer_equals_the_brute_force_on_seeded_records():
    rng = np.random.default_rng(22)
    recs = TS.seeded_records(rng, 900, 1500, 3200)
    assert {c for r in recs for _n, c in r[1]} == set(range(9))
    for region in REGIONS:
        got = statement(recs, region)
        assert got == brute(recs, region), region
        assert all(type(v) is int for v in got)
    first = statement(recs, REGIONS[0])
    assert all(v > 0 for v in first), first                       # every word is exercised
    assert statement(recs, REGIONS[7]) == [0] * 7 and statement(recs, REGIONS[5])[3:5] == [0, 0] and statement(recs, REGIONS[8])[3] == 0
    assert statement(recs, REGIONS[5])[5:] == first[5:]           # the cov words are counted whatever the mask


X0, X1 = 5000, 5600


def region(tol=T, nmin=300, nmax=1200, mask=ALL, mc=C, flank=F, gmin=G, x0=X0, x1=X1):
    return (min(x0, x1) - max(tol, flank) - 1, max(x0, x1) + max(tol, flank) + 1, x0, x1, tol, mc, nmin, nmax, mask, flank, gmin)


def one(ops, pos0, **kw):
    r = [(pos0, ops, 60, 0)]
    got = statement(r, region(**kw))
    assert got == brute(r, region(**kw)), (ops, pos0, kw)
    return got


def test_answer_at_the_edges_of_the_rule():
    x = X0
    far = 20000                                   # a second target nothing reaches
    # pos = x - F and x - F + 1; q = x + F and x + F - 1
    assert one([(400, M)], x - F, x1=far)[3:] == [1, 0, 1, 0] and one([(400, M)], x - F + 1, x1=far)[3:] == [0, 0, 1, 0]
    assert one([(400, M)], x + F - 400, x1=far)[3] == 1 and one([(400, M)], x + F - 1 - 400, x1=far)[3] == 0
    # a D of 40 that ends at a + n = x - F does not block, at x - F + 1 it does; one that starts at x + F - 1 does, at x + F not
    for end, ref in ((x - F, 1), (x - F + 1, 0)):
        assert one([(100, M), (40, D), (400, M)], end - 140, x1=far)[:4] == [0, 0, 0, ref]
    for start, ref in ((x + F - 1, 0), (x + F, 1)):
        assert one([(start - (x - 200), M), (40, N), (100, M)], x - 200, x1=far)[:4] == [0, 0, 0, ref]
    # an I of 40 at x - F - 1, x - F, x + F, x + F + 1
    for at, ref in ((x - F - 1, 1), (x - F, 0), (x, 0), (x + F, 0), (x + F + 1, 1)):
        assert one([(at - (x - 200), M), (40, I), (400, M)], x - 200, x1=far)[:4] == [0, 0, 0, ref]
    # lengths g - 1 and g, of a D and of an I in the middle
    for n, ref in ((G - 1, 1), (G, 0)):
        assert one([(200, M), (n, D), (200, M)], x - 200, x1=far)[3] == ref and one([(200, M), (n, I), (200, M)], x - 200, x1=far)[3] == ref
    # cov: pos <= x < q
    assert one([(10, M)], x, x1=far)[5] == 1 and one([(10, M)], x + 1, x1=far)[5] == 0
    assert one([(10, M)], x - 10, x1=far)[5] == 0 and one([(10, M)], x - 9, x1=far)[5] == 1
    # an I does not move the cursor, a D does; S, H and P neither: q is the reference end
    assert one([(40, S), (F, EQ), (5, I), (3, PAD), (F, X), (40, H)], x - F, x1=far, mc=100)[3] == 1
    assert one([(F, M), (5, I), (F - 1, M), (40, S)], x - F, x1=far, mc=100)[3] == 0
    # a record without operations, and the all-clip records
    assert one([], x) == [0] * 7 and one([(200, S)], x) == [0] * 7 and one([(100, H), (100, S)], x) == [0] * 7


def test_the_priority_of_the_classes():
    tandup = LC0 | RC1 | INSOP | REF0 | REF1
    # a record that is both cg and a spanner of both targets: a TANDUP's I in the middle of the interval
    rec = ([(500, M), (600, I), (500, M)], X0 - 200)
    assert one(*rec, mask=tandup) == [1, 0, 0, 0, 0, 1, 1]
    assert one(*rec, mask=tandup & ~INSOP) == [0, 0, 0, 1, 1, 1, 1]               # without the bit it is reference support
    assert one(*rec, mask=tandup, nmin=601) == [0, 0, 0, 1, 1, 1, 1]
    # tol >= F: a record that is clip_0 and span_0 counts as alt_l
    assert one([(40, S), (400, M)], X0 - 55, tol=60, mask=LC0 | REF0) == [0, 1, 0, 0, 0, 1, 0]
    assert one([(40, S), (400, M)], X0 - 55, tol=60, mask=REF0) == [0, 0, 0, 1, 0, 1, 0]
    assert one([(40, S), (400, M)], X0 - 55, tol=50, mask=LC0 | REF0) == [0, 0, 0, 1, 0, 1, 0]
    # cg wins over a clip: a counted D and a trailing clip at x1 in one record
    assert one([(200, M), (600, D), (40, M), (40, S)], X0 - 200, mask=GAP | RC1 | REF1) == [1, 0, 0, 0, 0, 1, 1]
    assert one([(200, M), (600, D), (40, M), (40, S)], X0 - 200, mask=RC1 | REF1) == [0, 0, 1, 0, 0, 1, 1]
    # both clips of one record count once each; bits 6 / 7 off: no reference word, the cov words stay
    assert one([(40, S), (600, M), (40, S)], X0, mask=LC0 | RC1) == [0, 1, 1, 0, 0, 1, 0]
    assert one([(1000, M)], X0 - 200, mask=63) == [0, 0, 0, 0, 0, 1, 1]
    assert one([(1000, M)], X0 - 200, mask=63 | REF0) == [0, 0, 0, 1, 0, 1, 1] and one([(1000, M)], X0 - 200, mask=63 | REF1) == [0, 0, 0, 0, 1, 1, 1]
    # x0 = x1: the two targets' words are one
    assert one([(1000, M)], X0 - 200, x1=X0) == [0, 0, 0, 1, 1, 1, 1] and one([(40, S), (300, M)], X0 + 3, x1=X0) == [0, 1, 1, 0, 0, 0, 0]
    # a GAP counted at the targets blocks both: the explicit priority changes nothing for it when g <= nmin and tol < F
    for off in (-T, 0, T):
        assert one([(300, M), (600, D), (300, M)], X0 + off - 300, mask=REF0 | REF1)[3:5] == [0, 0]


def test_bad_regions_are_refused():
    good = (100, 300, 200, 200, 50, 30, 0, 10, ALL, F, G)
    assert support.answer([], good) == [0] * 7
    for k, v in ((0, -1), (0, 301), (1, 1 << 31), (4, -1), (4, 256), (6, 11), (9, 0), (9, 65536), (10, 0)):
        bad = list(good)
        bad[k] = v
        assert not support.region_ok(bad)
        with pytest.raises(ValueError):
            support.answer([], bad)
    assert support.region_ok(good[:9] + (65535, 1 << 40))


def test_the_classes_are_disjoint():
    rng = np.random.default_rng(23)
    recs = TS.seeded_records(rng, 1500, 1500, 3200)
    regs = [r for t, loc in (("DEL", ["c", 2001, 2600]), ("TANDUP", ["c", 2001, 2500]), ("INV", ["c", 2201, 2400]), ("INS", ("c", 2300, 80)),
                             ("DEL", ["c", 2001, 2100])) for r in support.regions(t, loc, 10 ** 5)]
    seen = [0] * 7
    for rg in regs + REGIONS:
        own = rg in regs
        for rec in recs:
            w = statement([rec], rg)
            seen = [a + b for a, b in zip(seen, w)]
            # for any field values: a record is in one class at most at a target
            assert w[0] + w[1] <= 1 and w[0] + w[2] <= 1 and w[0] + w[3] <= 1 and w[0] + w[4] <= 1 and w[1] + w[3] <= 1 and w[2] + w[4] <= 1
            if own:
                # support.regions' own (tol < F, g <= nmin): a counted clip at target k excludes span_k, a counted GAP both -
                # only an INSOP leaves a spanner to the explicit priority
                f = support.facts(rec[0], [(n << 4) | c for n, c in rec[1]], rg)
                if f is not None and not rec[3] & 0x704:
                    assert not (f["clip"][0] and f["span"][0]) and not (f["clip"][1] and f["span"][1])
                    if not rg[8] & INSOP:
                        assert not (f["cg"] and (f["span"][0] or f["span"][1]))
    assert all(v > 0 for v in seen), seen


# ------------------------------------------------------------------------------------------------------------------------------
# the genotype
# ------------------------------------------------------------------------------------------------------------------------------
def test_genotype_of_hand_derivable_counts():
    assert support.genotype(0, 0) == (None, None)
    l95, l05, l5 = math.log10(0.95), math.log10(0.05), math.log10(0.5)
    for n in (1, 4, 12):
        # (0, n): L0 = n log .95, L1 = n log .5, L2 = n log .05: 0/0, second is 0/1
        assert support.genotype(0, n) == ("0/0", min(99, math.floor(10 * n * (l95 - l5))))
        assert support.genotype(n, 0) == ("1/1", min(99, math.floor(10 * n * (l95 - l5))))
        # (n, n): L0 = L2 = n (log .05 + log .95), L1 = 2 n log .5: 0/1
        assert support.genotype(n, n) == ("0/1", min(99, math.floor(10 * n * (2 * l5 - l05 - l95))))
    assert support.genotype(0, 4) == ("0/0", 11) and support.genotype(4, 4) == ("0/1", 28) and support.genotype(8, 0) == ("1/1", 22)
    # the cap at 99
    assert support.genotype(0, 35)[1] == 97 and support.genotype(0, 36)[1] == 99 and support.genotype(500, 500) == ("0/1", 99)
    # a tie goes to fewer alt alleles: L0 = L1 where ALT log .05 + REF log .95 = (ALT + REF) log .5 - made exact by another error rate
    old = support.ERR
    try:
        support.ERR = 0.5                         # every likelihood is (ALT + REF) log10 .5: all three tie
        assert support.genotype(3, 9) == ("0/0", 0) and support.genotype(9, 3) == ("0/0", 0)
    finally:
        support.ERR = old
    # L0 = L2 for ALT = REF with any error rate: 0/0 against 1/1 is never chosen over 0/1 at 0.05, but the order holds
    ls = (4 * l05 + 4 * l95, 8 * l5, 4 * l95 + 4 * l05)
    assert ls[0] == ls[2] < ls[1]


# ------------------------------------------------------------------------------------------------------------------------------
# the mode's surface
# ------------------------------------------------------------------------------------------------------------------------------
def test_payload_round_trip_and_columns():
    m = modes.SUPPORT
    assert m.pack(None) == [] and m.unpack(m.pack(None)) is None and m.unpack([]) is None
    for x in (support.Payload([4, 5, 0, 3, 4, 7, 5], "DEL", 3001, 9000), support.Payload([0, 0, 8, 0, 8, 0, 0], "TANDUP", 1, 300),
              support.Payload([16, 16, 0, 50, 9, 50, 9], "INV", (1 << 31) - 60, (1 << 31) - 1), support.Payload([0] * 7, "INS", 7, 7),
              support.Payload([(1 << 32) - 1] * 7, "INS", 700, 700)):
        flat = m.pack(x)
        assert flat and all(isinstance(v, float) for v in flat)
        back = m.unpack(flat)
        assert type(back) is support.Payload and list(back) == list(x) and (back.svtype, back.start, back.end) == (x.svtype, x.start, x.end)
        assert len(m.columns_many([x, None])[0]) == len(m.COLUMNS)
    assert len(m.COLUMNS) == len(m.INFO) == len(m.keys) == len(m.columns_many([None])[0]) == 9
    assert m.columns_many([None])[0] == ["."] * 9
    assert list(m.COLUMNS) == ["VaPoR_SUP_ALT", "VaPoR_SUP_REF", "VaPoR_SUP_REFL", "VaPoR_SUP_REFR", "VaPoR_SUP_COVL", "VaPoR_SUP_COVR", "VaPoR_SUP_VAF",
                               "VaPoR_SUP_GT", "VaPoR_SUP_GQ"]
    assert all(len(i) == 4 and i[3].endswith("(--support)") for i in m.INFO)
    assert [i[1] for i in m.INFO] == ["Integer"] * 6 + ["Float", "String", "Integer"]
    assert m.attr == "support" and tuple(m.keys) == tuple(m.COLUMNS) and m.skip_dot and not m.phased
    # ALT = alt_cg + max(alt_l, alt_r) = 7, REF = max(ref_l, ref_r) = 6: L1 = 13 log .5 = -3.913, L2 = 7 log .95 + 6 log .05 = -7.962
    assert m.columns_many([support.Payload([2, 4, 5, 3, 6, 9, 8], "DEL", 3001, 9000)]) == [["7", "6", "3", "6", "9", "8", "0.538", "0/1", "40"]]
    assert m.columns_many([support.Payload([0, 0, 0, 0, 0, 3, 3], "INV", 3001, 3300)]) == [["0", "0", "0", "0", "3", "3", ".", ".", "."]]
    # a TANDUP has its six counts and no verdict
    assert m.columns_many([support.Payload([8, 0, 0, 4, 4, 8, 8], "TANDUP", 3001, 3300)]) == [["8", "4", "4", "4", "8", "8", ".", ".", "."]]


def test_info_lines_and_record_keys_of_the_annotated_vcf(tmp_path, monkeypatch):
    # tests/test_modes_cpu.py's check of a mode's ##INFO lines and of a record's keys, with this mode among its modes
    monkeypatch.setitem(TM.MODES, "support", modes.SUPPORT)
    monkeypatch.setitem(TM.NUMBER_DOT, "support", set())
    monkeypatch.setitem(TM.TYPES, "support", ["Integer"] * 6 + ["Float", "String", "Integer"])
    TM.test_info_lines_and_record_keys_of_the_annotated_vcf("support", tmp_path)


def test_payload_of_one_and_of_two_regions():
    regs = support.regions("INV", ["c", 3001, 3700], 10 ** 5)
    p = support.payload("INV", ["c", 3001, 3700], regs, [[1, 2, 3, 4, 5, 6, 7]])
    assert list(p) == [1, 2, 3, 4, 5, 6, 7] and (p.svtype, p.start, p.end) == ("INV", 3001, 3700)
    regs = support.regions("DEL", ["c", 3001, 15000], 10 ** 5)
    # two regions: the right breakpoint's words are the second's target 0; the first's cov_1 and the second's target 1 are ignored
    p = support.payload("DEL", ["c", 3001, 15000], regs, [[2, 6, 90, 3, 91, 8, 92], [93, 7, 94, 5, 95, 9, 96]])
    assert list(p) == [2, 6, 7, 3, 5, 8, 9] and support.columns(p)[:6] == ["9", "5", "3", "5", "8", "9"]
    p = support.payload("INS", ("c", 3000, 250), support.regions("INS", ("c", 3000, 250), 10 ** 5), [[4, 0, 0, 4, 4, 8, 8]])
    assert (p.start, p.end) == (3000, 3000) and support.columns(p) == ["4", "4", "4", "4", "8", "8", "0.500", "0/1", "28"]
    assert support.payload("BND", ["c", 1, 2], [], []) is None and support.payload("DEL", ["c", 1, 2], [], []) is None
    assert support.merge_words([1, 2, 3, 4, 5, 6, 7], [1, 1, 1, 1, 1, 1, 0]) == [2, 3, 4, 5, 6, 7, 7]


# ------------------------------------------------------------------------------------------------------------------------------
# the native host reader
# ------------------------------------------------------------------------------------------------------------------------------
REFS = TS.REFS
Q = 20
FX0, FX1 = 50000, 50800


@pytest.fixture(scope="module")
def designed(tmp_path_factory):
    """A file of designed records around the breakpoints 50 000 and 50 800 of contig c, a contig without records, a contig with a
    few; the records as the model takes them, per contig."""
    rng = np.random.default_rng(10)
    rows = []
    # one spanner per flag: 0x4, 0x100, 0x200, 0x400 never count; 0x800, 0x10, 0x1 do
    for i, flag in enumerate((0x4, 0x100, 0x200, 0x400, 0x800, 0x10, 0x1, 0x904)):
        rows.append(("flag%x" % flag, 0, FX0 - 200 + i, [(400, M)], 60, flag))
    rows.append(("q_below", 0, FX0 - 150, [(300, M)], Q - 1, 0))
    rows.append(("q_at", 0, FX0 - 151, [(300, M)], Q, 0))
    rows.append(("no_cigar", 0, FX0, [], 60, 0))
    rows.append(("all_clip", 0, FX0, [(200, S)], 60, 0))
    rows.append(("both", 0, FX0 - 300, [(1400, EQ)], 60, 0))
    rows.append(("edge_pos", 0, FX0 - F, [(200, M)], 60, 0))
    rows.append(("edge_pos1", 0, FX0 - F + 1, [(200, M)], 60, 0))
    rows.append(("edge_q", 0, FX0 + F - 200, [(200, M)], 60, 0))
    rows.append(("edge_q1", 0, FX0 + F - 201, [(200, M)], 60, 0))
    rows.append(("gap", 0, FX0 - 200, [(203, M), (795, D), (200, M)], 60, 0))
    rows.append(("small_d", 0, FX0 - 200, [(190, M), (G - 1, D), (200, M)], 60, 0))
    rows.append(("block_d", 0, FX0 - 200, [(190, M), (G, N), (200, M)], 60, 0))
    rows.append(("block_i", 0, FX0 - 200, [(200 + F, M), (G, I), (200, M)], 60, 0))
    rows.append(("free_i", 0, FX0 - 200, [(200 + F + 1, M), (G, I), (200, M)], 60, 0))
    rows.append(("ins_mid", 0, FX0 - 150, [(550, M), (700, I), (600, M)], 60, 0))
    rows.append(("lclip", 0, FX1 + 2, [(12, H), (20, S), (300, M)], 60, 0))
    rows.append(("rclip", 0, FX0 - 300 + 7, [(300, M), (40, S)], 60, 0))
    # a CG:B,I record: 70 000 operations that end at FX1 with a trailing clip, a D at FX0 inside them
    long_ops = [(1, M) if j % 2 == 0 else (1, I) for j in range(69996)]
    rows.append(("long_cg", 0, FX0 - 34998, long_ops + [(800, D), (0, M), (33, S), (9, H)], 60, 0))
    for i in range(160):
        r = TS.seeded_records(rng, 1, FX0 - 1000, FX0 + 1200)[0]
        rows.append(("r%d" % i, 0) + r)
    for i in range(6):
        rows.append(("f%d" % i, 2, 3000 + 700 * i, [(35, S), (1000, M), (35, S)], 60, 0))
    d = tmp_path_factory.mktemp("support_files")
    path = str(d / "designed.bam")
    TS.write_rows(path, REFS, rows)
    by_tid = {t: [(r[2], r[3], r[4], r[5]) for r in rows if r[1] == t] for t in range(3)}
    return path, by_tid


FILE_REGIONS = [
    (FX0 - F, FX1 + F, FX0, FX1, T, C, 400, 1600, ALL, F, G),
    (FX0 - F, FX1 + F, FX0, FX1, T, C, 400, 1600, RC0 | LC1 | GAP | REF0 | REF1, F, G),
    (FX0 - F, FX1 + F, FX0, FX1, T, C, 400, 1600, LC0 | RC1 | INSOP | REF0 | REF1, F, G),
    (FX0 - 256, FX1 + 256, FX0, FX1, 255, 1, 0, NCAP, ALL, 20, 1),
    (FX0 - 1, FX0 + 1, FX0, FX0, 0, C, 0, NCAP, ALL, 1, 1),
    (FX0 - F, FX0 + F, FX0, FX1, T, C, 400, 1600, RC0 | GAP | REF0, F, G),
    (FX1 - F, FX1 + F, FX1, FX1, T, C, 0, 0, LC0 | REF0, F, G),
    (FX0, FX0, FX0, FX0, T, C, 0, 0, ALL, F, G),
    (0, 200000, FX0 - 500, FX0 + 900, 100, 20, 5, 100, ALL, 65535, 1 << 40),
    (0, 200000, FX0 - 500, FX0 + 900, 100, 20, 5, 100, ALL, 300, 50),
]


def python_statement(path, chrom, rg, flt=(0, 0)):
    b = bamio.BamFile(path)
    b.set_filter(*flt)
    recs = [(r[1], r[2]) for r in b.fetch_raw(chrom, rg[0] + 1, rg[1], exclude_more=support.EXCLUDE)] if rg[1] > rg[0] else []
    return support.answer(recs, rg)


@pytest.mark.parametrize("flt", [(0, 0), (0, 0x800), (Q, 0), (Q, 0x810)])
def test_native_reader_equals_the_statement_and_the_brute_force(designed, flt, monkeypatch):
    path, by_tid = designed
    monkeypatch.setenv("VAPOR_BAM_DEVICE", "0")
    be = seqio.InProcessBam()
    be.read_filter = flt
    chroms = ["c"] * len(FILE_REGIONS) + ["e", "f", "nowhere"]
    regions = FILE_REGIONS + [(0, 5000, 1000, 2000, T, C, 0, 0, ALL, F, G), (2900, 5000, 3100, 3800, T, C, 0, 0, ALL, F, G), (0, 30, 10, 20, 5, C, 0, 0, ALL, F, G)]
    got = be.support_many(None, path, chroms, regions)
    for chrom, rg, g in zip(chroms, regions, got):
        tid = {"c": 0, "e": 1, "f": 2}.get(chrom)
        want = brute(by_tid[tid], rg, *flt) if tid is not None else [0] * 7
        assert g == want == python_statement(path, chrom, rg, flt), (chrom, rg)
    assert got[len(FILE_REGIONS)] == [0] * 7 and got[-1] == [0] * 7 and got[7] == [0] * 7
    assert got[0][0] >= 3 and got[0][3] >= 3 and got[0][4] >= 1 and got[1][3] > got[0][3] - 1
    # the Python route of support_many (VAPOR_BAM_NATIVE=0, or a library without the entries) gives the same
    monkeypatch.setenv("VAPOR_BAM_NATIVE", "0")
    assert be.support_many(None, path, chroms, regions) == got
    monkeypatch.delenv("VAPOR_BAM_NATIVE")

    class Without:
        def __getattr__(self, name):
            if name in ("vapor_bam_support", "vapor_bam_support_device"):
                raise AttributeError(name)
            return getattr(L.load(), name)
    real = L.load()
    monkeypatch.setattr(L, "_lib", Without())
    called = []
    monkeypatch.setattr(bamio.BamFile, "support_native", lambda self, *a, **k: called.append(a))
    assert seqio.InProcessBam.support_many(be, None, path, chroms, regions) == got and not called
    monkeypatch.setattr(L, "_lib", real)


def test_what_never_counts_and_what_the_user_decides(designed):
    path, by_tid = designed
    b = bamio.BamFile(path)
    tid = b.tid["c"]
    designed_only = by_tid[0][:27]
    rest = by_tid[0][27:]
    at_x0 = (FX0 - F, FX0 + F, FX0, FX1, T, C, 400, 1600, RC0 | GAP | REF0, F, G)

    def count(rg, flt=(0, 0), k=3):
        b.set_filter(*flt)
        return b.support_native(tid, rg)[k] - brute(rest, rg, *flt)[k]
    # the spanners: flags 0x800, 0x10, 0x1 of the eight; q_below and q_at; both, edge_pos, edge_q, small_d, free_i, ins_mid
    assert count(at_x0) == 3 + 2 + 6 == brute(designed_only, at_x0)[3]
    assert count(at_x0, (0, 0x800)) == 10 and count(at_x0, (0, 0x811)) == 8
    assert [count(at_x0, (q, 0)) for q in (0, Q, Q + 1)] == [11, 10, 9]
    # rclip ends at FX0 + 7: alt_l; the D of 795 and the D of 800 inside the CG:B,I record: alt_cg
    assert count(at_x0, k=1) == 1 and count(at_x0, k=0) == 2
    b.set_filter(0, 0)
    want = b.support_native(tid, FILE_REGIONS[0])
    b.set_dedup(True)
    assert b.support_native(tid, FILE_REGIONS[0]) == want == brute(by_tid[0], FILE_REGIONS[0])
    b.close()


def test_native_reader_refuses_bad_regions(designed):
    path, _ = designed
    b = bamio.BamFile(path)
    ch = [(b.first_record, b.first_record + 1)]
    good = (100, 300, 200, 200, 50, 30, 0, 10, ALL, F, G)
    assert b.support_native(0, good, ch) == [0] * 7
    for k, v in ((0, -1), (0, 301), (1, 1 << 31), (4, -1), (4, 256), (6, 11), (9, 0), (9, 65536), (10, 0)):
        bad = list(good)
        bad[k] = v
        with pytest.raises(ValueError, match="vapor_bam_support"):
            b.support_native(0, bad, ch)
    with pytest.raises(ValueError):
        b.support_native(-1, good, ch)
    b.close()


def test_abi_surface():
    h = open(os.path.join(ROOT, "include", "vapor_hip.h")).read()
    for name in ("vapor_bam_support", "vapor_bam_support_device"):
        assert re.search(r"\bint %s\(" % name, h) and name in L.EXPORTS and name in L.OPTIONAL_EXPORTS and hasattr(L.load(), name)
    assert L.ABI_VERSION == 3


# ------------------------------------------------------------------------------------------------------------------------------
# the stand-alone programs under the sanitizers
# ------------------------------------------------------------------------------------------------------------------------------
SAN = TS.SAN


def test_sup_pass_under_sanitizers_on_good_and_damaged_files(designed, tmp_path):
    exe = str(tmp_path / "bam_check")
    r = subprocess.run(["g++"] + SAN + ["-o", exe, os.path.join(ROOT, "tools", "bam_check.cpp"), "-lz", "-lpthread"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(path, first, win, *more):
        p = subprocess.run([exe, path, str(first), "0", str(win[0]), str(win[1]), "200", "2"] + [str(m) for m in more], env=env,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, (path, p.returncode, p.stderr[-2000:])
        return p.stdout.splitlines()
    path, by_tid = designed
    first = bamio.BamFile(path).first_record
    # every record of the file walked, a region per contig: the words are the brute force's
    for flt in ((), (Q, 0x800)):
        out = [ln for ln in run(path, first, (FX0, FX1), *flt, "sup") if ln.startswith("sup:")]
        assert len(out) == 2
        for t, ln in enumerate(out):
            want = brute(by_tid[t], (0, (1 << 31) - 1, FX0, FX1, 50, 30, 0, 1 << 28, 255, 51, 30), *(flt or (0, 0)))
            f = ln.split()
            assert f[:6] == ["sup:", "contig", str(t), "rc", "0", "words"] and [int(x) for x in f[6:13]] == want, ln
        assert all(int(x) > 0 for x in out[0].split()[6:13])
    assert not any(ln.startswith("sup:") for ln in run(path, first, (FX0, FX1)))
    # the damaged files of tests/test_bamio.py: a status, never a report
    small = TB._small_bam(tmp_path)
    first = bamio.BamFile(small).first_record
    assert run(small, first, (4000, 5500), "sup")[-1].startswith("sup: contig 1 rc 0 words ")
    raw = open(small, "rb").read()
    off, bsize, xlen = TB._blocks(raw)[6]
    n_err = 0
    for field in ("isize_huge", "isize_small", "bsize_tiny", "bsize_big", "crc", "payload_bit", "xlen_big", "truncated"):
        b = bytearray(raw)
        if field == "isize_huge":
            struct.pack_into("<I", b, off + bsize - 4, 0xFFFFFFFF)
        elif field == "isize_small":
            struct.pack_into("<I", b, off + bsize - 4, 17)
        elif field == "bsize_tiny":
            struct.pack_into("<H", b, off + 16, 9)
        elif field == "bsize_big":
            struct.pack_into("<H", b, off + 16, 0xFFFF)
        elif field == "crc":
            b[off + bsize - 8] ^= 0x40
        elif field == "payload_bit":
            b[off + 12 + xlen + (bsize - xlen - 20) // 2] ^= 0x04
        elif field == "xlen_big":
            struct.pack_into("<H", b, off + 10, 0xFFF0)
        else:
            b = b[:off + bsize // 2]
        bad = str(tmp_path / ("v_%s.bam" % field))
        open(bad, "wb").write(bytes(b))
        lines = [ln for ln in run(bad, first, (4000, 5500), "sup") if ln.startswith("sup: contig 0 rc ")]
        assert len(lines) == 1, lines
        n_err += lines[0].startswith("sup: contig 0 rc -4")
    assert n_err >= 7, n_err              # (a file cut between two blocks may end like one without EOF marker)


def test_the_plan_of_the_device_call_under_sanitizers():
    lines = readplan_program.output().splitlines()
    assert lines[-1] == "readplan_check: all equal"
    sup = [ln for ln in lines if ln.startswith("support plan: ")]
    assert len(sup) == 1 and "clamped fields and collected words equal the rule" in sup[0] and 'both size refusals say "in one call"' in sup[0]
    assert int(sup[0].split()[2]) == 1000 and int(re.search(r"\((\d+) refused\)", sup[0]).group(1)) > 1000


# ------------------------------------------------------------------------------------------------------------------------------
# cli.main on a world whose columns are known
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def fake(oracle):
    pipeline.set_engine(FakeEngine(oracle))
    yield
    pipeline.set_engine(None)
    seqio.set_backend(None)


LAYERS = 3
SHORT = 2000


def closed_form(specs, layers=LAYERS, short=SHORT):
    """The nine columns of every locus of make_support_world from its parameters, with A alt haplotypes (0 ref, 1 het, 2 hom) of
    `layers` layers each.  ALT: one record a layer and alt haplotype carries the event in its CIGAR (an event of at most `short`
    bases, not INV), or one is clipped at each breakpoint (longer) - two at each for an INV, the forward and the reverse-strand
    piece.  REF: one spanner a layer and reference haplotype at each breakpoint - and, for a TANDUP that is split, one a layer
    and alt haplotype as well (the duplicated allele holds both outer breakpoints with their neighbours).  COV: the spanners
    and the alt records that hold the breakpoint's base - the D or I carrier (2 * layers in all); of a split read the piece
    that starts at the breakpoint, not the one that ends there: a split DEL's left base is held by the reference reads alone,
    a split TANDUP's by its spanners and the piece that starts there."""
    out = []
    for t, span, zyg in specs:
        a = {"ref": 0, "het": 1, "hom": 2}[zyg]
        split = span > short or t == "INV"
        alt = a * layers * (2 if t == "INV" else 1)
        ref = 2 * layers if t == "TANDUP" and split else (2 - a) * layers
        covl = covr = 2 * layers
        if t == "DEL" and split:
            covl = (2 - a) * layers
        if t == "TANDUP" and split:
            covl = (2 + a) * layers
        cols = [str(alt), str(ref), str(ref), str(ref), str(covl), str(covr)]
        if t == "TANDUP":
            cols += [".", ".", "."]
        else:
            ls = sorted([alt * math.log10(0.05) + ref * math.log10(0.95), (alt + ref) * math.log10(0.5), alt * math.log10(0.95) + ref * math.log10(0.05)])
            cols += ["%.3f" % (alt / (alt + ref)), ("0/0", "0/1", "1/1")[a], str(min(99, math.floor(10 * (ls[2] - ls[1]))))]
        out.append(cols)
    return out


def locus_of(l):
    return (l.chrom, l.start, len(l.ins_seq)) if l.svtype == "INS" else [l.chrom, l.start, l.end]


@pytest.mark.parametrize("kw", [{}, {"layers": 4, "read_len": 700, "guard": F}, {"layers": 2, "margin": 2500, "short": 700}])
def test_the_reference_statement_gives_the_closed_form_on_every_locus(kw):
    w = synth.make_support_world(seed=6, **dict({"layers": LAYERS}, **kw))
    expect = closed_form(synth.SUPPORT_SPECS, layers=kw.get("layers", LAYERS), short=kw.get("short", SHORT))
    assert len(w.loci) == len(synth.SUPPORT_SPECS) == len(expect) == 24
    mem = seqio.MemorySamtools(w)
    for l, spec, e in zip(w.loci, synth.SUPPORT_SPECS, expect):
        regs = support.regions(l.svtype, locus_of(l), len(w.contigs[l.chrom]))
        assert len(regs) == (2 if spec[1] > P and spec[0] != "INS" else 1)
        got = mem.support_many(None, "x", [l.chrom] * len(regs), regs)
        assert support.columns(support.payload(l.svtype, locus_of(l), regs, got)) == e, (spec, got, e)
    # every type short and long, every zygosity; the existing worlds are what they were (their own tests hold them to their forms)
    assert {(t, s > kw.get("short", SHORT), z) for t, s, z in synth.SUPPORT_SPECS} == {(t, b, z) for t in support.TYPES for b in (False, True) for z in ("het", "hom", "ref")}
    for rs in w.reads.values():
        for r in rs:
            assert sum(o >> 4 for o in signature.parse_cigar(r.cigar) if o & 15 in (0, 1, 4, 7, 8)) == len(r.seq), r.qname


def test_closed_form_of_the_world_by_hand():
    by = {s: c for s, c in zip(synth.SUPPORT_SPECS, closed_form(synth.SUPPORT_SPECS, layers=4))}
    assert by[("DEL", 600, "het")] == ["4", "4", "4", "4", "8", "8", "0.500", "0/1", "28"]
    assert by[("DEL", 12000, "hom")] == ["8", "0", "0", "0", "0", "8", "1.000", "1/1", "22"]
    assert by[("INV", 700, "het")] == ["8", "4", "4", "4", "8", "8", "0.667", "0/1", "17"]
    assert by[("INS", 3000, "ref")] == ["0", "8", "8", "8", "8", "8", "0.000", "0/0", "22"]
    assert by[("TANDUP", 300, "het")] == ["4", "4", "4", "4", "8", "8", ".", ".", "."]
    assert by[("TANDUP", 15000, "hom")] == ["8", "8", "8", "8", "16", "8", ".", ".", "."]


def test_cli_on_a_support_world_in_memory(fake, tmp_path):
    w = synth.make_support_world(seed=4, layers=LAYERS)
    expect = closed_form(synth.SUPPORT_SPECS)
    text = synth.bed_text(w)
    seqio.set_backend(seqio.MemorySamtools(w))
    plain, _ = TS.run_main(tmp_path, "plain", "bed", text)
    seqio.set_backend(seqio.MemorySamtools(w))
    table, _ = TS.run_main(tmp_path, "sup", "bed", text, ["--support"])
    rows = [r.split("\t") for r in table.splitlines()]
    assert rows[0][-9:] == list(support.COLUMNS)
    # the row's own columns are the plain run's, byte for byte; a plain run has no column of the mode
    assert "\n".join("\t".join(r[:-9]) for r in rows) + "\n" == plain and "VaPoR_SUP" not in plain
    assert len(rows) == len(w.loci) + 1
    for r, l, e in zip(rows[1:], w.loci, expect):
        assert r[-9:] == e, (l, r[-9:], e)
    # 0x800 excluded: the supplementary half of every split read is gone; --dedup-qname has no effect on the counts
    seqio.set_backend(seqio.MemorySamtools(w))
    flt, _ = TS.run_main(tmp_path, "flt", "bed", text, ["--support", "--exclude-flags", "0x800", "--dedup-qname", "--min-mapq", "5"])
    frows = [r.split("\t") for r in flt.splitlines()]
    k = synth.SUPPORT_SPECS.index(("DEL", 600, "het"))
    assert frows[k + 1][-9:] == expect[k]                                # a D carrier has no supplementary record
    k = synth.SUPPORT_SPECS.index(("DEL", 12000, "hom"))
    assert int(frows[k + 1][-9]) <= int(expect[k][0]) and frows[k + 1][-8:-5] == expect[k][1:4]
    # vcf: DEL, INV and INS records get the INFO keys, the '.' ones left out; TANDUP is not scored by `vapor vcf`
    vtext = synth.vcf_text(w)
    seqio.set_backend(seqio.MemorySamtools(w))
    vplain, _ = TS.run_main(tmp_path, "vplain", "vcf", vtext)
    seqio.set_backend(seqio.MemorySamtools(w))
    vtable, annotated = TS.run_main(tmp_path, "vsup", "vcf", vtext, ["--support"])
    vrows = [r.split("\t") for r in vtable.splitlines()]
    assert "\n".join("\t".join(r[:-9]) for r in vrows) + "\n" == vplain
    by_chrom = {r[0].split(":")[0]: r[-9:] for r in vrows[1:]}
    n_seen = 0
    for l, e in zip(w.loci, expect):
        if l.svtype != "TANDUP":
            assert by_chrom[l.chrom] == e, l
            n_seen += 1
    assert n_seen == 18
    lines = annotated.splitlines()
    assert sum(ln.startswith("##INFO=<ID=VaPoR_SUP_") for ln in lines) == 9
    rec = {ln.split("\t")[2]: ln.split("\t")[7] for ln in lines if not ln.startswith("#")}
    assert rec["sg1"].endswith(";VaPoR_SUP_ALT=3;VaPoR_SUP_REF=3;VaPoR_SUP_REFL=3;VaPoR_SUP_REFR=3;VaPoR_SUP_COVL=6;VaPoR_SUP_COVR=6;"
                               "VaPoR_SUP_VAF=0.500;VaPoR_SUP_GT=0/1;VaPoR_SUP_GQ=21")
    assert set(rec) == {l.svid for l in w.loci if l.svtype != "TANDUP"} and all("VaPoR_SUP_GT=" in v for v in rec.values())


def test_the_sam_text_backends_take_column_six():
    """SamtoolsCLI / SamtoolsHybrid: POS and CIGAR of `view`'s lines behind _sam_fields' filter, lengths from the .fai."""
    w = synth.make_support_world(seed=5, layers=2)
    mem = seqio.MemorySamtools(w)

    class Text(seqio.SamtoolsCLI):
        def __init__(self):
            self.read_filter = (0, 0)

        def view_lines(self, bam, region):
            return mem.view_lines(bam, region)

        def fai_lines(self, ref):
            return mem.fai_lines(ref)
    txt = Text()
    for flt in ((0, 0), (0, 0x800)):
        txt.read_filter = mem.read_filter = flt
        for l in w.loci:
            regs = support.regions(l.svtype, locus_of(l), txt.contig_length("x", "r", l.chrom))
            got = txt.support_many(None, "x", [l.chrom] * len(regs), regs)
            assert got == mem.support_many(None, "x", [l.chrom] * len(regs), regs) and sum(got[0]) > 0

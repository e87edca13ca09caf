"""`vapor bed | vcf --signatures` without a GPU: the parser, the regions of a locus (signature.regions), the events
of a record and a region's answer (signature.events / answer) against a brute-force statement written here - every record
expanded to one operation code per position, the events found in the expansion - the native host reader (vapor_bam_signature)
against both on files written case by case, tools/bam_check.cpp's sig pass and tools/readplan_check.cpp under the sanitizers as
programs of their own, the mode's surface, and cli.main on a world whose six columns are known in closed form
(synth.make_signature_world).  Device work of the row's own columns is answered by tests/fake_engine.py (oracle-backed, test
only).  Every comparison is on integers and exact."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import readplan_program
import test_bamio as TB
import test_modes_cpu as TM
from fake_engine import FakeEngine
from vapor_amd import _lib as L
from vapor_amd import bamio, cli, modes, pipeline, seqio, signature, synth
from vapor_amd import simple_function as SF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--sv-input", "a.bed", "--reference", "r.fa", "--pacbio-input", "x.bam", "--output-path", "o", "--output-file", "o.vapor"]
C, T, P = 30, 50, 10000
NCAP = (1 << 28) - 1


# ------------------------------------------------------------------------------------------------------------------------------
# the parser
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_parser_takes_signatures_on_bed_and_vcf():
    assert cli.build_parser().parse_args(BASE).signatures is False
    assert cli.build_parser().parse_args(BASE + ["--signatures"]).signatures is True
    assert cli.build_parser().parse_args(BASE + ["--signatures", "--min-mapq", "20", "--exclude-flags", "0x800", "--dedup-qname", "--bnd",
                                                 "--no-figures"]).signatures is True
    m = modes.SIGNATURES
    assert m.name == "signatures" and m.chunk_payloads is not None and m.chunk_gens is None
    assert tuple(TM.hook_payloads(m)) == signature.TYPES          # the hook answers for the module's types
    assert (signature.C, signature.T, signature.P, signature.EXCLUDE) == (C, T, P, 0x704)


@pytest.mark.parametrize("cmd, more, message", [
    ("bed", ["--signatures", "--refine", "20"], "--signatures and --refine cannot be combined"),
    ("vcf", ["--signatures", "--phased"], "--signatures and --phased cannot be combined"),
    ("bed", ["--signatures", "--phase-vcf", "p.vcf"], "--signatures and --phase-vcf cannot be combined"),
    ("vcf", ["--signatures", "--both-ends"], "--signatures and --both-ends cannot be combined"),
    ("bed", ["--signatures", "--depth"], "--signatures and --depth cannot be combined"),
    ("svelter", ["--signatures"], "--signatures applies to `vapor bed` and `vapor vcf`"),
    ("ins", ["--signatures"], "--signatures applies to `vapor bed` and `vapor vcf`"),
])
def test_refused_option_combinations(cmd, more, message, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main([cmd] + BASE + more)
    assert e.value.code == 2 and message in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------------------------------------
# signature.regions
# ------------------------------------------------------------------------------------------------------------------------------
LC0, RC0, LC1, RC1, GAP, INSOP = 1, 2, 4, 8, 16, 32
MASKS = {"DEL": RC0 | LC1 | GAP, "TANDUP": LC0 | RC1 | INSOP, "INV": 15, "INS": RC0 | LC1 | INSOP}


@pytest.mark.parametrize("svtype", ["DEL", "TANDUP", "INV"])
def test_regions_at_the_split_threshold(svtype):
    n = 10 ** 6
    s = 50000
    mask = MASKS[svtype]
    # J1 - J0 = e - (s - 1) = P: one region
    e = s - 1 + P
    nmin, nmax = (max(30, (P + 1) // 2), 2 * P) if svtype != "INV" else (0, 0)
    assert signature.regions(svtype, ["c", s, e], n) == [(s - 1 - T - 1, e + T + 1, s - 1, e, T, C, nmin, nmax, mask)]
    # P + 1: two, the second with x0 = x1 = J1 and bits 0 / 1 for what bits 2 / 3 mean; GAP in the first only, INSOP in neither
    e += 1
    first, second = signature.regions(svtype, ["c", s, e], n)
    length = P + 1
    gap = svtype == "DEL"
    assert first == (s - 1 - T - 1, s - 1 + T + 1, s - 1, e, T, C, max(30, (length + 1) // 2) if gap else 0, 2 * length if gap else 0,
                     mask & (LC0 | RC0 | GAP))
    assert second == (e - T - 1, e + T + 1, e, e, T, C, 0, 0, (mask >> 2) & 3)
    assert not (first[8] | second[8]) & INSOP


def test_regions_of_an_insertion_and_of_the_other_types():
    n = 10 ** 6
    # an INS has one breakpoint: J1 - J0 = 0 whatever its length; the bounds are computed on len
    for length in (P, P + 1, 5 * P):
        assert signature.regions("INS", ("c", 7000, length), n) == [(7000 - T - 1, 7000 + T + 1, 7000, 7000, T, C, max(30, (length + 1) // 2), 2 * length,
                                                                     MASKS["INS"])]
    assert signature.regions("INS", ("c", 7000, 1 << 28), n)[0][6:8] == (1 << 27, NCAP)         # clamped
    assert signature.regions("INS", ("c", 7000, 1 << 30), n)[0][6:8] == (NCAP, NCAP)
    assert signature.regions("DEL", ["c", 1000, 1000 + (1 << 29)], 1 << 30)[0][6:8] == (NCAP, NCAP)
    for t in ("BND", "DISDUP", "DEL_INV", "DUP_INV", "Other"):
        assert signature.regions(t, ["c", 500, 900], n) == []


def test_regions_at_both_ends_of_a_contig_and_with_one_base():
    # the left end: J0 - T - 1 < 0; the right end: J1 + T + 1 beyond the contig; a contig the file does not have
    assert signature.regions("DEL", ["c", 10, 400], 5000)[0][:4] == (0, 400 + T + 1, 9, 400)
    assert signature.regions("DEL", ["c", 1, 400], 5000)[0][:4] == (0, 451, 0, 400)
    assert signature.regions("INV", ["c", 4000, 4990], 5000)[0][:4] == (3999 - T - 1, 5000, 3999, 4990)
    assert signature.regions("TANDUP", ["c", 4000, 5000], 5000)[0][:4] == (3948, 5000, 3999, 5000)
    assert signature.regions("DEL", ["c", 4000, 4500], 0)[0][:2] == (0, 0)
    assert signature.regions("INS", ("c", 0, 100), 5000)[0][:4] == (0, T + 1, 0, 0)
    assert signature.regions("INS", ("c", 5000, 100), 5000)[0][:4] == (5000 - T - 1, 5000, 5000, 5000)
    far = signature.regions("DEL", ["c", 100, 100 + 3 * P], 2 * P)
    assert [r[:2] for r in far] == [(99 - T - 1, 99 + T + 1), (2 * P, 2 * P)]                  # the second window is empty
    # L = 1: nmin = max(30, 1) = 30 is above nmax = 2, so no operation can count - the bit is off and the bounds ascend
    for t in ("DEL", "TANDUP", "INS"):
        r = signature.regions(t, ["c", 700, 700] if t != "INS" else ("c", 700, 1), 5000)
        assert len(r) == 1 and r[0][6:8] == (0, 0) and r[0][8] == MASKS[t] & 15
    assert signature.regions("DEL", ["c", 700, 700], 5000)[0][:6] == (699 - T - 1, 700 + T + 1, 699, 700, T, C)
    assert signature.regions("DEL", ["c", 700, 713], 5000)[0][6:9] == (0, 0, MASKS["DEL"] & 15)            # L = 14: 2 L = 28 < 30
    assert signature.regions("DEL", ["c", 700, 714], 5000)[0][6:9] == (30, 30, MASKS["DEL"])               # L = 15: 30 = 2 L counts
    assert signature.regions("DEL", ["c", 700, 715], 5000)[0][6:9] == (30, 32, MASKS["DEL"])
    for t in MASKS:
        for loc in (["c", 2, 30000], ["c", 700, 900], ["c", 4990, 5100]):
            for r in signature.regions(t, loc, 5000):
                assert 0 <= r[0] <= r[1] <= 5000 and r[6] <= r[7] and r[4] == T and r[5] == C


# ------------------------------------------------------------------------------------------------------------------------------
# signature.events / answer against a brute-force statement
# ------------------------------------------------------------------------------------------------------------------------------
ADVANCES = {0, 2, 3, 7, 8}         # M D N = X
CLIPS = {4, 5}


def brute_events(pos0, ops, min_clip):
    """The model: the record as one operation code per position of its CIGAR, and the events read off that expansion.  (Made
    for records as a BAM file holds them: no operation of length 0, no two equal codes in a row, at most two clip operations
    at an end.)"""
    x = [code for n, code in ops for _ in range(n)]
    if not x or all(c in CLIPS for c in x):
        return []
    out = []
    lead = next(i for i, c in enumerate(x) if c not in CLIPS)
    trail = next(i for i, c in enumerate(reversed(x)) if c not in CLIPS)
    if lead >= max(min_clip, 1):
        out.append(("LCLIP", pos0))
    cur, i = pos0, 0
    while i < len(x):
        j = i
        while j < len(x) and x[j] == x[i]:
            j += 1
        if x[i] in (2, 3):
            out.append(("GAP", cur, j - i))
        elif x[i] == 1:
            out.append(("INSOP", cur, j - i))
        if x[i] in ADVANCES:
            cur += j - i
        i = j
    if trail >= max(min_clip, 1):
        out.append(("RCLIP", cur))
    return out


def brute(records, region, min_mapq=0, exclude=0):
    """A region's ten words from the model's events.  records: (pos0, [(n, code)...], mapq, flag)."""
    w0, w3, x0, x1, tol, min_clip, nmin, nmax, mask = region
    counts = [0] * 6
    offs = ([], [])
    for pos0, ops, mapq, flag in records:
        if mapq < min_mapq or flag & (exclude | 0x704) or pos0 >= w3 or w3 <= w0:
            continue
        for ev in brute_events(pos0, ops, min_clip):
            if ev[0] == "LCLIP" or ev[0] == "RCLIP":
                for k, x in enumerate((x0, x1)):
                    bit = 2 * k + (ev[0] == "RCLIP")
                    if mask >> bit & 1 and -tol <= ev[1] - x <= tol:
                        counts[bit] += 1
                        offs[k].append(ev[1] - x)
            elif ev[0] == "GAP":
                if mask & GAP and nmin <= ev[2] <= nmax and abs(ev[1] - x0) <= tol and abs(ev[1] + ev[2] - x1) <= tol:
                    counts[4] += 1
                    offs[0].append(ev[1] - x0)
                    offs[1].append(ev[1] + ev[2] - x1)
            elif mask & INSOP and nmin <= ev[2] <= nmax and x0 - tol <= ev[1] <= x1 + tol:
                counts[5] += 1
                if abs(ev[1] - x0) <= tol:
                    offs[0].append(ev[1] - x0)
    out = list(counts)
    for k in (0, 1):
        if not offs[k]:
            out += [0, 0]
            continue
        # the largest count, then the smallest |offset|, then the negative one
        best = sorted(set(offs[k]), key=lambda o: (-offs[k].count(o), abs(o), o))[0]
        out += [best, offs[k].count(best)]
    return out


def as_records(records):
    return [(pos0 + 1, np.asarray([(n << 4) | c for n, c in ops], dtype=np.uint32)) for pos0, ops, _q, _f in records]


def statement(records, region, min_mapq=0, exclude=0):
    kept = [r for r in records if not (r[2] < min_mapq or r[3] & (exclude | 0x704))]
    return signature.words(signature.answer(as_records(kept), region))


def seeded_records(rng, n, lo, hi, clip_p=0.5):
    """Records as a file holds them, every operation code among them: a body of M I D N P = X without two equal codes in a
    row, and at each end none, one or two clip operations (H outside S)."""
    recs = []
    for _ in range(n):
        body, last = [], -1
        for _k in range(int(rng.integers(1, 14))):
            code = int(rng.choice([0, 1, 2, 3, 6, 7, 8]))
            if code == last:
                continue
            body.append((int(rng.integers(1, 120)), code))
            last = code
        lead = [(int(rng.integers(1, 45)), c) for c in ((), (4,), (5,), (5, 4))[int(rng.integers(0, 4))]] if rng.random() < clip_p else []
        trail = [(int(rng.integers(1, 45)), c) for c in ((), (4,), (5,), (4, 5))[int(rng.integers(0, 4))]] if rng.random() < clip_p else []
        recs.append((int(rng.integers(lo, hi)), lead + body + trail, int(rng.integers(0, 61)), int(rng.choice([0, 0, 0, 16, 0x800, 0x400, 0x100]))))
    return recs


REGIONS = [
    (1900, 3200, 2000, 3000, 50, 30, 1, 500, 63),
    (1900, 2200, 2050, 2050, 50, 30, 1, NCAP, 63),                # x0 == x1
    (0, 9000, 2500, 2600, 255, 1, 0, NCAP, 63),                   # the widest tolerance, every clip
    (2400, 2700, 2500, 2600, 0, 10, 0, NCAP, 63),                 # tol 0
    (1900, 3200, 2000, 3000, 50, 30, 40, 80, GAP | INSOP),
    (1900, 3200, 2000, 3000, 50, 30, 0, 0, 15),
    (1900, 3200, 2000, 3000, 50, 30, 1, 500, 0),                  # nothing counts
    (2500, 2500, 2450, 2450, 40, 30, 1, 500, 63),                 # an empty window
    (1949, 2051, 2000, 6000, 50, 30, 1, NCAP, RC0 | GAP),         # the first region of a long event
]


def test_events_and_answer_equal_the_brute_force_on_seeded_records():
    rng = np.random.default_rng(20)
    recs = seeded_records(rng, 900, 1500, 3200)
    assert {c for r in recs for _n, c in r[1]} == set(range(9))
    for pos0, ops, _q, _f in recs[:300]:
        packed = [(n << 4) | c for n, c in ops]
        for mc in (1, 30, 44):
            assert signature.events(pos0, packed, mc) == brute_events(pos0, ops, mc), (pos0, ops, mc)
    for region in REGIONS:
        got = statement(recs, region)
        assert got == brute(recs, region), region
        assert all(isinstance(x, int) for x in got)
    assert sum(statement(recs, REGIONS[0])[:6]) > 20 and statement(recs, REGIONS[6]) == [0] * 10 == statement(recs, REGIONS[7])


def test_events_on_designed_records():
    M, I, D, N, S, H, PAD, EQ, X = range(9)

    def ev(ops, mc=C, pos0=1000, model=True):
        got = signature.events(pos0, [(n << 4) | c for n, c in ops], mc)
        if model and all(n > 0 for n, _c in ops):
            assert got == brute_events(pos0, ops, mc), ops
        return got
    assert ev([]) == [] and ev([(500, M)]) == []
    assert ev([(30, S), (500, M)]) == [("LCLIP", 1000)] and ev([(29, S), (500, M)]) == []
    assert ev([(500, M), (30, H)]) == [("RCLIP", 1500)] and ev([(500, M), (29, H)]) == []
    # H + S reach C only together, at either end
    assert ev([(10, H), (20, S), (500, EQ), (14, S), (16, H)]) == [("LCLIP", 1000), ("RCLIP", 1500)]
    assert ev([(10, H), (19, S), (500, M), (13, S), (16, H)]) == []
    # a record of at most two operations that are all clips has neither event
    assert ev([(100, S)]) == [] and ev([(100, H), (100, S)]) == [] and ev([(100, S), (100, S)]) == []
    # D and N are GAPs at the cursor where they start; I is an INSOP there; I S H P do not move it
    assert ev([(100, M), (40, D), (50, X), (7, I), (60, N), (5, PAD), (10, EQ)]) == [("GAP", 1100, 40), ("INSOP", 1190, 7), ("GAP", 1190, 60)]
    assert ev([(40, S), (100, M), (25, I), (100, M), (50, D), (100, M), (35, S)]) == [
        ("LCLIP", 1000), ("INSOP", 1100, 25), ("GAP", 1200, 50), ("RCLIP", 1350)]
    # only the first two and the last two operations are read for a clip (no valid file has more: the model is not asked)
    assert ev([(10, S), (10, S), (10, S), (5, M)], mc=25, model=False) == [] and ev([(10, S), (15, S), (10, S), (5, M)], mc=25, model=False) == [("LCLIP", 1000)]
    assert ev([(5, M), (10, H), (10, S), (10, S)], mc=25, model=False) == [] and ev([(100, S), (100, S), (100, H)], model=False) == [("LCLIP", 1000), ("RCLIP", 1000)]
    # an operation of length 0 is one: a 0D is a GAP of length 0, and min_clip below 1 still needs a clipped base
    assert ev([(5, M), (0, D), (5, M)]) == [("GAP", 1005, 0)] and ev([(0, S), (5, M)], mc=0) == [] and ev([(1, S), (5, M)], mc=-3) == [("LCLIP", 1000)]


def test_answer_on_designed_regions():
    M, I, D, S, H = 0, 1, 2, 4, 5
    x0, x1 = 5000, 5600

    def region(tol=T, nmin=300, nmax=1200, mask=63, mc=C):
        return (x0 - tol - 1, x1 + tol + 1, x0, x1, tol, mc, nmin, nmax, mask)

    def one(ops, pos0, **kw):
        r = [(pos0, ops, 60, 0)]
        got = statement(r, region(**kw))
        assert got == brute(r, region(**kw))
        return got
    # every bit at the offsets -T - 1, -T, 0, T, T + 1
    for off, counted in ((-T - 1, 0), (-T, 1), (0, 1), (T, 1), (T + 1, 0)):
        assert one([(40, S), (100, M)], x0 + off)[:6] == [counted, 0, 0, 0, 0, 0]
        assert one([(100, M), (40, S)], x0 + off - 100)[:6] == [0, counted, 0, 0, 0, 0]
        assert one([(40, S), (100, M)], x1 + off)[:6] == [0, 0, counted, 0, 0, 0]
        assert one([(100, M), (40, H)], x1 + off - 100)[:6] == [0, 0, 0, counted, 0, 0]
        assert one([(100, M), (600, D), (100, M)], x0 + off - 100)[:6] == [0, 0, 0, 0, counted, 0]
        assert one([(100, M), (600 - off, D), (100, M)], x0 + off - 100)[4] == (1 if abs(off) <= T else 0)      # the right end stays at x1
        assert one([(100, M), (600 + 2 * off, D), (100, M)], x0 - off - 100)[4] == (1 if abs(off) <= T else 0)
        assert one([(100, M), (400, I), (100, M)], x0 + off - 100)[:6] == [0, 0, 0, 0, 0, 1 if off >= -T else 0]    # anywhere up to x1 + T
        assert one([(100, M), (400, I), (100, M)], x1 + off - 100)[5] == (1 if off <= T else 0)
    # n at nmin - 1, nmin, nmax, nmax + 1
    for n, counted in ((599, 0), (600, 1), (640, 1), (641, 0)):
        assert one([(100, M), (n, D), (100, M)], x0 - 100, nmin=600, nmax=640)[4] == counted
        assert one([(100, M), (n, I), (100, M)], x0 - 100, nmin=600, nmax=640)[5] == counted
    # every mask bit alone, and none
    both = [(x0, [(40, S), (560, M), (600, D), (40, M), (33, I), (600 - 40, M), (40, S)], 60, 0)]
    # (the record: LCLIP at x0, a D of 600 from x0 + 560, an I of 33 at x0 + 1200, RCLIP at x0 + 1760)
    for bit, targets in ((0, (x0, x1)), (1, (x0 + 1760, x1)), (2, (x0 - 900, x0)), (3, (x0, x0 + 1760)), (4, (x0 + 560, x0 + 1160)), (5, (x0 + 1150, x0 + 1250))):
        r = (x0 - 1000, x0 + 2000, targets[0], targets[1], 50, C, 20, 1200, 1 << bit)
        want = [0] * 6
        want[bit] = 1
        assert statement(both, r)[:6] == brute(both, r)[:6] == want, bit
        for other in range(6):
            if other != bit:
                r2 = r[:8] + (1 << other,)
                assert statement(both, r2)[bit] == 0 and statement(both, r2) == brute(both, r2)
    assert statement(both, (x0 - 700, x1 + 700, x0, x1, 50, C, 20, 1200, 0)) == [0] * 10
    # clip sums of C - 1 and C
    assert one([(C - 1, S), (100, M)], x0)[0] == 0 and one([(C, S), (100, M)], x0)[0] == 1
    assert one([(C - 10, H), (9, S), (100, M)], x0)[0] == 0 and one([(C - 10, H), (10, S), (100, M)], x0)[0] == 1


def test_the_mode_and_its_ties():
    S, M = 4, 0
    x0 = 7000
    region = (x0 - 100, x0 + 100, x0, x0 + 5000, 60, C, 0, 0, LC0)

    def mode(offsets):
        recs = [(x0 + o, [(40, S), (200, M)], 60, 0) for o in offsets]
        got = statement(recs, region)
        assert got == brute(recs, region)
        assert got[0] == len(offsets) and got[8:] == [0, 0]
        return got[6:8]
    assert mode([]) == [0, 0]
    assert mode([17]) == [17, 1] and mode([-60]) == [-60, 1] and mode([60]) == [60, 1]              # one event, and the edges
    assert mode([3, 3, -9, -9, -9, 20]) == [-9, 3]                                                   # the largest count wins
    assert mode([5, 5, -2, -2, 30, 30]) == [-2, 2]                                                   # a tie: the smallest |offset|
    assert mode([4, -4]) == [-4, 1] and mode([-4, 4, 4, -4]) == [-4, 2]                              # then the negative offset
    assert mode([0, 1, -1]) == [0, 1] and mode([1, -1, 2, -2]) == [-1, 1]
    assert mode([60, -60, 59]) == [59, 1]
    assert signature.mode_of([0, 2, 0, 2, 0], 2) == (-1, 2) and signature.mode_of([0] * 5, 2) == (0, 0)


# ------------------------------------------------------------------------------------------------------------------------------
# the native host reader
# ------------------------------------------------------------------------------------------------------------------------------
CODES = "MIDNSHP=X"
REFS = [("c", 200000), ("e", 5000), ("f", 20000)]
Q = 20


def cigar_text(ops):
    return "".join("%d%s" % (n, CODES[c]) for n, c in ops) or "*"


def seq_len(ops):
    return sum(n for n, c in ops if c in (0, 1, 4, 7, 8))


def write_rows(path, refs, rows, block_size=8192):
    """rows: (name, tid, pos0, ops, mapq, flag).  The bases are not looked at."""
    recs = []
    for name, tid, pos0, ops, mapq, flag in rows:
        n = seq_len(ops)
        recs.append((name, tid, pos0, cigar_text(ops), "ACGT" * (n // 4) + "ACGT"[:n % 4], None, mapq, flag))
    bamio.write_bam(path, refs, recs, block_size=block_size)


X0, X1 = 50000, 50800


@pytest.fixture(scope="module")
def designed(tmp_path_factory):
    """A file of designed records around the breakpoints 50 000 and 50 800 of contig c, a contig without records, a contig with a
    few; the records as the model takes them, per contig."""
    rng = np.random.default_rng(9)
    M, I, D, N, S, H = 0, 1, 2, 3, 4, 5
    rows = []
    # one clipped record per flag: 0x4, 0x100, 0x200, 0x400 never count; 0x800, 0x10, 0x1 do
    for i, flag in enumerate((0x4, 0x100, 0x200, 0x400, 0x800, 0x10, 0x1, 0x904)):
        rows.append(("flag%x" % flag, 0, X0 + i - 4, [(40, S), (300, M)], 60, flag))
    rows.append(("q_below", 0, X0 - 300 + 7, [(300, M), (40, S)], Q - 1, 0))
    rows.append(("q_at", 0, X0 - 300 + 9, [(300, M), (40, S)], Q, 0))
    rows.append(("no_cigar", 0, X0, [], 60, 0))
    rows.append(("h_and_s", 0, X1 + 2, [(12, H), (20, S), (300, M)], 60, 0))
    rows.append(("s_and_h_short", 0, X1 + 3, [(12, H), (17, S), (300, M)], 60, 0))
    rows.append(("all_clip", 0, X0, [(200, S)], 60, 0))
    rows.append(("all_clip2", 0, X0, [(100, H), (100, S)], 60, 0))
    rows.append(("gap", 0, X0 - 200, [(203, M), (795, D), (200, M)], 60, 0))
    rows.append(("gapN", 0, X0 - 250, [(251, M), (801, N), (200, M)], 60, 0))
    rows.append(("ins", 0, X0 - 150, [(400, M), (700, I), (100, M)], 60, 0))
    # a CG:B,I record: 70 000 operations that end at X1 with a trailing clip, a GAP at X0 inside them
    long_ops = [(1, M) if j % 2 == 0 else (1, I) for j in range(69996)]
    rows.append(("long_cg", 0, X0 - 34998, long_ops + [(800, D), (0, M), (33, S), (9, H)], 60, 0))
    for i in range(160):
        r = seeded_records(rng, 1, X0 - 1000, X0 + 1200)[0]
        rows.append(("r%d" % i, 0) + r)
    for i in range(6):
        rows.append(("f%d" % i, 2, 3000 + 700 * i, [(35, S), (1000, M), (35, S)], 60, 0))
    d = tmp_path_factory.mktemp("signature_files")
    path = str(d / "designed.bam")
    write_rows(path, REFS, rows)
    by_tid = {t: [(r[2], r[3], r[4], r[5]) for r in rows if r[1] == t] for t in range(3)}
    return path, by_tid


FILE_REGIONS = [
    (X0 - T - 1, X1 + T + 1, X0, X1, T, C, 400, 1600, 63),
    (X0 - T - 1, X1 + T + 1, X0, X1, T, C, 400, 1600, RC0 | LC1 | GAP),
    (X0 - 256, X1 + 256, X0, X1, 255, 1, 0, NCAP, 63),
    (X0 - 1, X0 + 1, X0, X0, 0, C, 0, NCAP, 63),
    (X0 - T - 1, X0 + T + 1, X0, X1, T, C, 400, 1600, RC0 | GAP),
    (X1 - T - 1, X1 + T + 1, X1, X1, T, C, 0, 0, LC0),
    (X0, X0, X0, X0, T, C, 0, 0, 63),
    (0, 200000, X0 - 500, X0 + 900, 100, 20, 5, 100, 63),
]


def python_statement(path, chrom, region, flt=(0, 0)):
    b = bamio.BamFile(path)
    b.set_filter(*flt)
    recs = [(r[1], r[2]) for r in b.fetch_raw(chrom, region[0] + 1, region[1], exclude_more=signature.EXCLUDE)] if region[1] > region[0] else []
    return signature.words(signature.answer(recs, region))


@pytest.mark.parametrize("flt", [(0, 0), (0, 0x800), (Q, 0), (Q, 0x810)])
def test_native_reader_equals_the_statement_and_the_brute_force(designed, flt, monkeypatch):
    path, by_tid = designed
    monkeypatch.setenv("VAPOR_BAM_DEVICE", "0")
    be = seqio.InProcessBam()
    be.read_filter = flt
    chroms = ["c"] * len(FILE_REGIONS) + ["e", "f", "nowhere"]
    regions = FILE_REGIONS + [(0, 5000, 1000, 2000, T, C, 0, 0, 63), (2900, 3100, 3000, 3000, T, C, 0, 0, 63), (0, 30, 10, 20, 5, C, 0, 0, 63)]
    got = be.signature_many(None, path, chroms, regions)
    for chrom, rg, g in zip(chroms, regions, got):
        tid = {"c": 0, "e": 1, "f": 2}.get(chrom)
        want = brute(by_tid[tid], rg, *flt) if tid is not None else [0] * 10
        assert g == want == python_statement(path, chrom, rg, flt), (chrom, rg)
    assert got[len(FILE_REGIONS)] == [0] * 10 and got[-1] == [0] * 10 and got[len(FILE_REGIONS) + 1][0] == 1
    assert got[6] == [0] * 10 and got[0][4] >= 2 and got[0][5] >= 1
    # the Python route of signature_many (VAPOR_BAM_NATIVE=0, or a library without the entries) gives the same
    monkeypatch.setenv("VAPOR_BAM_NATIVE", "0")
    assert be.signature_many(None, path, chroms, regions) == got
    monkeypatch.delenv("VAPOR_BAM_NATIVE")

    class Without:
        def __getattr__(self, name):
            if name in ("vapor_bam_signature", "vapor_bam_signature_device"):
                raise AttributeError(name)
            return getattr(L.load(), name)
    real = L.load()
    monkeypatch.setattr(L, "_lib", Without())
    called = []
    monkeypatch.setattr(bamio.BamFile, "signature_native", lambda self, *a, **k: called.append(a))
    assert seqio.InProcessBam.signature_many(be, None, path, chroms, regions) == got and not called
    monkeypatch.setattr(L, "_lib", real)


def test_what_never_counts_and_what_the_user_decides(designed):
    path, by_tid = designed
    b = bamio.BamFile(path)
    tid = b.tid["c"]
    designed_only = by_tid[0][:19]
    rest = by_tid[0][19:]
    lclip = (X0 - T - 1, X0 + T + 1, X0, X0, T, C, 0, 0, LC0)

    def count(region, flt=(0, 0), k=0):
        b.set_filter(*flt)
        return b.signature_native(tid, region)[k] - brute(rest, region, *flt)[k]
    # of the eight flag records 0x800, 0x10 and 0x1 count (0x904 holds 0x100 and 0x4)
    assert count(lclip) == 3 == brute(designed_only, lclip)[0]
    assert count(lclip, (0, 0x800)) == 2 and count(lclip, (0, 0x811)) == 0
    # MAPQ Q - 1 is dropped at --min-mapq Q, Q is kept: the two records end at X0 + 7 and X0 + 9
    rclip = (X0 - T - 1, X0 + T + 1, X0, X0, T, C, 0, 0, RC0)
    assert [count(rclip, (q, 0), 1) for q in (0, Q, Q + 1)] == [2, 1, 0]
    b.set_filter(0, 0)
    assert b.signature_native(tid, rclip)[6:8] == brute(by_tid[0], rclip)[6:8]
    # H + S reach C together (12 + 20), 12 + 17 do not; the all-clip records and the one without CIGAR have no event
    at_x1 = (X1 - T - 1, X1 + T + 1, X1, X1, T, C, 0, 0, LC0)
    assert count(at_x1) == 1
    # the D of 795 at X0 + 3, the N of 801 at X0 + 1, the D of 800 inside the CG:B,I record at X0, whose trailing clip is at X1
    gaps = (X0 - T - 1, X1 + T + 1, X0, X1, T, C, 400, 1600, GAP | RC1)
    assert count(gaps, k=4) == 3 and count(gaps, k=3) == 1
    want = b.signature_native(tid, FILE_REGIONS[0])
    b.set_dedup(True)
    assert b.signature_native(tid, FILE_REGIONS[0]) == want == brute(by_tid[0], FILE_REGIONS[0])
    b.close()


def test_native_reader_refuses_bad_regions(designed):
    path, _ = designed
    b = bamio.BamFile(path)
    ch = [(b.first_record, b.first_record + 1)]
    good = (100, 300, 200, 200, 50, 30, 0, 10, 63)
    assert b.signature_native(0, good, ch) == [0] * 10
    for k, v in ((0, -1), (0, 301), (1, 1 << 31), (4, -1), (4, 256), (6, 11)):
        bad = list(good)
        bad[k] = v
        with pytest.raises(ValueError, match="vapor_bam_signature"):
            b.signature_native(0, bad, ch)
    with pytest.raises(ValueError):
        b.signature_native(-1, good, ch)
    b.close()


def test_abi_surface():
    h = open(os.path.join(ROOT, "include", "vapor_hip.h")).read()
    for name in ("vapor_bam_signature", "vapor_bam_signature_device"):
        assert re.search(r"\bint %s\(" % name, h) and name in L.EXPORTS and name in L.OPTIONAL_EXPORTS and hasattr(L.load(), name)
    assert L.ABI_VERSION == 3


# ------------------------------------------------------------------------------------------------------------------------------
# the stand-alone programs under the sanitizers
# ------------------------------------------------------------------------------------------------------------------------------
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
       "-I" + os.path.join(ROOT, "vapor_amd", "csrc")]


def test_sig_pass_under_sanitizers_on_good_and_damaged_files(designed, tmp_path):
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
        out = [ln for ln in run(path, first, (X0, X1), *flt, "sig") if ln.startswith("sig:")]
        assert len(out) == 2
        for t, ln in enumerate(out):
            want = brute(by_tid[t], (0, (1 << 31) - 1, X0, X1, 50, 30, 0, 1 << 28, 63), *(flt or (0, 0)))
            f = ln.split()
            assert f[:5] == ["sig:", "contig", str(t), "rc", "0"] and [int(x) for x in f[6:12]] == want[:6] and [int(x) for x in f[13:17]] == want[6:], ln
        assert sum(int(x) for x in out[0].split()[6:12]) > 5
    assert not any(ln.startswith("sig:") for ln in run(path, first, (X0, X1)))
    # the damaged files of tests/test_bamio.py: a status, never a report
    small = TB._small_bam(tmp_path)
    first = bamio.BamFile(small).first_record
    assert run(small, first, (4000, 5500), "sig")[-1].startswith("sig: contig 1 rc 0 counts ")
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
        lines = [ln for ln in run(bad, first, (4000, 5500), "sig") if ln.startswith("sig: contig 0 rc ")]
        assert len(lines) == 1, lines
        n_err += lines[0].startswith("sig: contig 0 rc -4")
    assert n_err >= 7, n_err              # (a file cut between two blocks may end like one without EOF marker)


def test_the_plan_of_the_device_call_under_sanitizers():
    lines = readplan_program.output().splitlines()
    assert lines[-1] == "readplan_check: all equal"
    sig = [ln for ln in lines if ln.startswith("signature plan: ")]
    assert len(sig) == 1 and "clamped fields and collected words equal the rule" in sig[0] and 'both size refusals say "in one call"' in sig[0]
    assert int(sig[0].split()[2]) == 1500 and int(re.search(r"\((\d+) refused\)", sig[0]).group(1)) > 1000


# ------------------------------------------------------------------------------------------------------------------------------
# the mode's surface
# ------------------------------------------------------------------------------------------------------------------------------
def test_payload_round_trip_and_columns():
    m = modes.SIGNATURES
    assert m.pack(None) == [] and m.unpack(m.pack(None)) is None and m.unpack([]) is None
    for x in (signature.Payload([4, 5, 0, -3, 4, 7, 5], "DEL", 3001, 9000), signature.Payload([0, 0, 8, 0, 8, 0, 0], "TANDUP", 1, 300),
              signature.Payload([16, 16, 0, -50, 9, 50, 9], "INV", (1 << 31) - 60, (1 << 31) - 1), signature.Payload([0, 0, 0, 0, 0, 0, 0], "INS", 7, 7),
              signature.Payload([(1 << 32) - 1, 1, (1 << 32) - 1, -255, 1, 255, 1], "INS", 700, 700)):
        flat = m.pack(x)
        assert flat and all(isinstance(v, float) for v in flat)
        back = m.unpack(flat)
        assert type(back) is signature.Payload and list(back) == list(x) and (back.svtype, back.start, back.end) == (x.svtype, x.start, x.end)
        assert len(m.columns_many([x, None])[0]) == len(m.COLUMNS)
    assert len(m.COLUMNS) == len(m.INFO) == len(m.keys) == len(m.columns_many([None])[0]) == 6
    assert m.columns_many([None])[0] == ["."] * 6
    assert list(m.COLUMNS) == ["VaPoR_SIG_L", "VaPoR_SIG_R", "VaPoR_SIG_CG", "VaPoR_SIG_N", "VaPoR_SIG_POS", "VaPoR_SIG_END"]
    assert all(len(i) == 4 and i[1] == "Integer" and i[3].endswith("(--signatures)") for i in m.INFO)
    assert m.attr == "signatures" and tuple(m.keys) == tuple(m.COLUMNS) and m.skip_dot and not m.phased
    # N = CG + max(L, R); POS = start + off0, END = end + off1; '.' without a mode
    assert m.columns_many([signature.Payload([4, 5, 2, -3, 4, 7, 5], "DEL", 3001, 9000)]) == [["4", "5", "2", "7", "2998", "9007"]]
    assert m.columns_many([signature.Payload([0, 0, 8, 0, 8, 0, 0], "TANDUP", 3001, 3300)]) == [["0", "0", "8", "8", "3001", "."]]
    assert m.columns_many([signature.Payload([0, 0, 0, 0, 0, 0, 0], "INV", 3001, 3300)]) == [["0", "0", "0", "0", ".", "."]]


def test_payload_of_one_and_of_two_regions():
    regs = signature.regions("INV", ["c", 3001, 3700], 10 ** 5)
    p = signature.payload("INV", ["c", 3001, 3700], regs, [[1, 2, 3, 4, 0, 0, -2, 3, 5, 4]])
    assert list(p) == [3, 7, 0, -2, 3, 5, 4] and (p.svtype, p.start, p.end) == ("INV", 3001, 3700)
    regs = signature.regions("DEL", ["c", 3001, 15000], 10 ** 5)
    p = signature.payload("DEL", ["c", 3001, 15000], regs, [[0, 6, 0, 0, 2, 0, 1, 5, 0, 2], [7, 0, 0, 0, 0, 0, -1, 7, 0, 0]])
    assert list(p) == [6, 7, 2, 1, 5, -1, 7] and signature.columns(p) == ["6", "7", "2", "9", "3002", "14999"]
    # an INS has one breakpoint: its two modes are one, the better by the tie rule
    regs = signature.regions("INS", ("c", 3000, 250), 10 ** 5)
    p = signature.payload("INS", ("c", 3000, 250), regs, [[0, 2, 3, 0, 0, 4, 2, 4, -1, 5]])
    assert list(p) == [2, 3, 4, -1, 5, -1, 5] and signature.columns(p) == ["2", "3", "4", "7", "2999", "2999"]
    assert signature.payload("BND", ["c", 1, 2], [], []) is None and signature.payload("DEL", ["c", 1, 2], [], []) is None
    assert signature.merge_words([1, 2, 3, 4, 5, 6, 3, 2, -3, 2], [1, 1, 1, 1, 1, 1, -3, 2, 9, 1]) == [2, 3, 4, 5, 6, 7, -3, 2, -3, 2]
    assert signature.merge_words([0] * 10, [0, 0, 0, 0, 0, 0, 0, 0, 4, 1]) == [0, 0, 0, 0, 0, 0, 0, 0, 4, 1]


# ------------------------------------------------------------------------------------------------------------------------------
# cli.main on a world whose columns are known
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def fake(oracle):
    pipeline.set_engine(FakeEngine(oracle))
    yield
    pipeline.set_engine(None)
    seqio.set_backend(None)


def run_main(tmp_path, name, mode, text, more=(), fa="ref.fa", bam="x.bam"):
    d = tmp_path / name
    d.mkdir()
    src = d / ("in." + mode)
    src.write_text(text)
    out = d / "out.vapor"
    args = [mode, "--sv-input", str(src), "--reference", fa, "--pacbio-input", bam, "--output-path", str(d / "figs"),
            "--output-file", str(out), "--no-figures"] + list(more)
    seen = {}
    orig = SF.vcf_vapor_modify

    def keep_table(vcf_input, rec_new, *a, **k):
        seen["table"] = open(vcf_input + ".vapor").read()
        return orig(vcf_input, rec_new, *a, **k)
    SF.vcf_vapor_modify = keep_table
    try:
        assert cli.main(args) == 0
    finally:
        SF.vcf_vapor_modify = orig
    table = seen["table"] if mode == "vcf" else out.read_text()
    annotated = open(str(src) + ".vapor").read() if mode == "vcf" else None
    return table, annotated


LAYERS = 4
JITTER = (0, 2, -2, 2)


def closed_form(w, specs, layers=LAYERS, jitter=JITTER, short=2000):
    """The six columns of every locus of make_signature_world from its parameters.  With A alt haplotypes (1 het, 2 hom) there
    are A * layers reads at each junction.  An event of at most `short` bases (not INV) is carried in the CIGAR: CG = A * layers,
    no clips; a longer DEL, TANDUP or INS is split: L = R = A * layers; an INV shows two clips at each breakpoint per read:
    L = R = 2 * A * layers.  The offsets: layer k reports its breakpoints jitter[k] to the right - on the reverse strand of an
    inversion that is jitter[k] to the left, so an INV's histograms hold both signs - and the mode is the tie rule's."""
    out = []
    for l, (t, span, zyg) in zip(w.loci, specs):
        a = 2 if zyg == "hom" else 1
        offs = [jitter[k % len(jitter)] for k in range(layers)] * a
        if t == "INV":
            offs = offs + [-o for o in offs]
        best = sorted(set(offs), key=lambda o: (-offs.count(o), abs(o), o))[0]
        n = a * layers
        if t == "INS":
            cols = ["0", "0", str(n), str(n)] if span <= short else [str(n), str(n), "0", str(n)]
            out.append(cols + [str(l.start + best)] * 2)
        elif t == "INV":
            out.append([str(2 * n), str(2 * n), "0", str(2 * n), str(l.start + best), str(l.end + best)])
        elif span <= short:
            # (a short TANDUP's I is left-aligned at the first breakpoint: nothing is said about the second)
            out.append(["0", "0", str(n), str(n), str(l.start + best), str(l.end + best) if t == "DEL" else "."])
        else:
            out.append([str(n), str(n), "0", str(n), str(l.start + best), str(l.end + best)])
    return out


def test_closed_form_of_the_world_by_hand():
    # the rule above, spelled out once for the default parameters: jitter (0, 2, -2, 2) has the mode +2 (two of four), and an
    # INV's histogram {0: 2, 2: 3, -2: 3} per haplotype-set ties at |2|, which the negative offset wins
    w = synth.make_signature_world(seed=4, layers=LAYERS, jitter=JITTER)
    cf = closed_form(w, synth.SIGNATURE_SPECS)
    by = {(t, span): c for (t, span, _z), c in zip(synth.SIGNATURE_SPECS, cf)}
    assert by[("DEL", 600)] == ["0", "0", "8", "8", "3003", "3602"] and by[("DEL", 6000)] == ["4", "4", "0", "4", "3003", "9002"]
    assert by[("DEL", 12000)] == ["8", "8", "0", "8", "3003", "15002"] and by[("TANDUP", 300)] == ["0", "0", "4", "4", "3003", "."]
    assert by[("TANDUP", 15000)] == ["4", "4", "0", "4", "3003", "18002"] and by[("INV", 700)] == ["8", "8", "0", "8", "2999", "3698"]
    assert by[("INV", 11000)] == ["16", "16", "0", "16", "2999", "13998"]
    assert by[("INS", 250)] == ["0", "0", "4", "4", "3002", "3002"] and by[("INS", 3000)] == ["8", "8", "0", "8", "3002", "3002"]
    spans = [l.end - (l.start - 1) for l in w.loci if l.svtype != "INS"]
    assert any(s <= P for s in spans) and any(s > P for s in spans)
    flags = {r.flag for rs in w.reads.values() for r in rs}
    assert {0, 0x10, 0x800, 0x810} <= flags
    assert any(re.search(r"\d+D", r.cigar) for rs in w.reads.values() for r in rs) and any("I" in r.cigar for rs in w.reads.values() for r in rs)
    # every record's CIGAR spells its bases
    for rs in w.reads.values():
        for r in rs:
            assert sum(o >> 4 for o in signature.parse_cigar(r.cigar) if o & 15 in (0, 1, 4, 7, 8)) == len(r.seq), r.qname


def test_cli_on_a_signature_world_in_memory(fake, tmp_path):
    w = synth.make_signature_world(seed=4, layers=LAYERS, jitter=JITTER)
    expect = closed_form(w, synth.SIGNATURE_SPECS)
    text = synth.bed_text(w)
    seqio.set_backend(seqio.MemorySamtools(w))
    plain, _ = run_main(tmp_path, "plain", "bed", text)
    seqio.set_backend(seqio.MemorySamtools(w))
    table, _ = run_main(tmp_path, "sig", "bed", text, ["--signatures"])
    rows = [r.split("\t") for r in table.splitlines()]
    assert rows[0][-6:] == list(signature.COLUMNS)
    # the row's own columns are the plain run's, byte for byte
    assert "\n".join("\t".join(r[:-6]) for r in rows) + "\n" == plain
    assert len(rows) == len(w.loci) + 1
    for r, l, e in zip(rows[1:], w.loci, expect):
        assert r[-6:] == e, (l, r[-6:], e)
    # a plain run does not depend on the option's existence: the mode is none and the table has no column of it
    assert "VaPoR_SIG" not in plain
    # 0x800 excluded: the supplementary half of every split read is gone, the primary half stays
    seqio.set_backend(seqio.MemorySamtools(w))
    flt_plain, _ = run_main(tmp_path, "flt_plain", "bed", text, ["--exclude-flags", "0x800", "--dedup-qname", "--min-mapq", "5"])
    seqio.set_backend(seqio.MemorySamtools(w))
    flt, _ = run_main(tmp_path, "flt", "bed", text, ["--signatures", "--exclude-flags", "0x800", "--dedup-qname", "--min-mapq", "5"])
    frows = [r.split("\t") for r in flt.splitlines()]
    assert "\n".join("\t".join(r[:-6]) for r in frows) + "\n" == flt_plain
    assert frows[1][-6:] == expect[0]                                    # a D carrier has no supplementary record
    k = [i for i, s in enumerate(synth.SIGNATURE_SPECS) if s[:2] == ("DEL", 6000)][0]
    assert int(frows[k + 1][-6]) + int(frows[k + 1][-5]) == int(expect[k][0])
    # vcf: DEL, INV and INS records get the INFO keys; TANDUP is not scored by `vapor vcf`
    vtext = synth.vcf_text(w)
    seqio.set_backend(seqio.MemorySamtools(w))
    vplain, _ = run_main(tmp_path, "vplain", "vcf", vtext)
    seqio.set_backend(seqio.MemorySamtools(w))
    vtable, annotated = run_main(tmp_path, "vsig", "vcf", vtext, ["--signatures"])
    vrows = [r.split("\t") for r in vtable.splitlines()]
    assert "\n".join("\t".join(r[:-6]) for r in vrows) + "\n" == vplain
    by_chrom = {r[0].split(":")[0]: r[-6:] for r in vrows[1:]}
    for l, e in zip(w.loci, expect):
        if l.svtype != "TANDUP":
            assert by_chrom[l.chrom] == e, l
    lines = annotated.splitlines()
    assert sum(ln.startswith("##INFO=<ID=VaPoR_SIG_") for ln in lines) == 6
    rec = {ln.split("\t")[2]: ln.split("\t")[7] for ln in lines if not ln.startswith("#")}
    assert rec["sg1"].endswith(";VaPoR_SIG_L=0;VaPoR_SIG_R=0;VaPoR_SIG_CG=8;VaPoR_SIG_N=8;VaPoR_SIG_POS=3003;VaPoR_SIG_END=3602")
    assert rec["sg9"].endswith(";VaPoR_SIG_L=16;VaPoR_SIG_R=16;VaPoR_SIG_CG=0;VaPoR_SIG_N=16;VaPoR_SIG_POS=2999;VaPoR_SIG_END=13998")
    assert set(rec) == {l.svid for l in w.loci if l.svtype != "TANDUP"} and all("VaPoR_SIG_N=" in v for v in rec.values())


def test_the_sam_text_backends_take_column_six():
    """SamtoolsCLI / SamtoolsHybrid: POS and CIGAR of `view`'s lines behind _sam_fields' filter, lengths from the .fai."""
    w = synth.make_signature_world(seed=5, layers=3, jitter=(1, -1))
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
            n = txt.contig_length("x", "r", l.chrom)
            locus = (l.chrom, l.start, len(l.ins_seq)) if l.svtype == "INS" else [l.chrom, l.start, l.end]
            regs = signature.regions(l.svtype, locus, n)
            got = txt.signature_many(None, "x", [l.chrom] * len(regs), regs)
            assert got == mem.signature_many(None, "x", [l.chrom] * len(regs), regs) and sum(got[0][:6]) > 0

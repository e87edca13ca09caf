"""`vapor bed | vcf --depth` without a GPU: the parser, the interval rule (depth.regions), what a record covers
(depth.cover) against a per-base pile-up stated here, the native host reader (vapor_bam_depth) against both on files written
case by case, tools/bam_check.cpp's depth pass under the sanitizers on good and damaged files, the mode's surface as cli.py and
the VCF writer see it, and cli.main on a world whose depth is known in closed form (synth.make_depth_world).  Device work of the
row's own columns is answered by tests/fake_engine.py (oracle-backed, test only)."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import test_bamio as TB
from fake_engine import FakeEngine
from vapor_amd import _lib as L
from vapor_amd import bamio, cli, depth, modes, pipeline, seqio, synth
from vapor_amd import simple_function as SF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--sv-input", "a.bed", "--reference", "r.fa", "--pacbio-input", "x.bam", "--output-path", "o", "--output-file", "o.vapor"]
W, P = 1000, 10000


# ------------------------------------------------------------------------------------------------------------------------------
# the parser
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_parser_takes_depth_on_bed_and_vcf():
    assert cli.build_parser().parse_args(BASE).depth is False
    assert cli.build_parser().parse_args(BASE + ["--depth"]).depth is True
    assert cli.build_parser().parse_args(BASE + ["--depth", "--min-mapq", "20", "--exclude-flags", "0x800", "--dedup-qname", "--bnd", "--no-figures"]).depth is True
    assert modes.DEPTH.name == "depth" and modes.DEPTH.chunk_payloads is not None and modes.DEPTH.chunk_gens is None
    assert modes.PHASED.chunk_payloads is None and modes.BOTH_ENDS.chunk_payloads is None and modes.refine(50, 10).chunk_payloads is None


@pytest.mark.parametrize("cmd, more, message", [
    ("bed", ["--depth", "--refine", "20"], "--depth and --refine cannot be combined"),
    ("vcf", ["--depth", "--phased"], "--depth and --phased cannot be combined"),
    ("bed", ["--depth", "--phase-vcf", "p.vcf"], "--depth and --phase-vcf cannot be combined"),
    ("vcf", ["--depth", "--both-ends"], "--depth and --both-ends cannot be combined"),
    ("svelter", ["--depth"], "--depth applies to `vapor bed` and `vapor vcf`"),
    ("ins", ["--depth"], "--depth applies to `vapor bed` and `vapor vcf`"),
])
def test_refused_option_combinations(cmd, more, message, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main([cmd] + BASE + more)
    assert e.value.code == 2 and message in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------------------------------------
# depth.regions
# ------------------------------------------------------------------------------------------------------------------------------
def test_regions_rule():
    n = 10 ** 6
    s = 50000
    # L = 1, 2P, 2P + 1
    assert depth.regions("DEL", ["c", s, s], n) == [(s - 1 - W, s - 1, s, s + W)]
    assert depth.regions("TANDUP", ["c", s, s + 2 * P - 1], n) == [(s - 1 - W, s - 1, s + 2 * P - 1, s + 2 * P - 1 + W)]
    e = s + 2 * P
    assert depth.regions("DEL", ["c", s, e], n) == [(s - 1 - W, s - 1, s - 1 + P, s - 1 + P), (e - P, e - P, e, e + W)]
    # the probes of a long event are P bases each, whatever its length
    for r in depth.regions("DEL", ["c", s, s + 5000000], 10 ** 7):
        assert r[2] - r[1] == P and (r[1] - r[0]) + (r[3] - r[2]) == W
    # s - 1 - W < 0; an event that starts at base 1 (a left flank clipped to length 0); e + W beyond the contig; a right flank of 0
    assert depth.regions("DEL", ["c", 301, 400], n) == [(0, 300, 400, 1400)]
    assert depth.regions("DEL", ["c", 1, 400], n) == [(0, 0, 400, 1400)]
    assert depth.regions("DEL", ["c", 5000, 5400], 5900) == [(3999, 4999, 5400, 5900)]
    assert depth.regions("DEL", ["c", 5000, 5400], 5400) == [(3999, 4999, 5400, 5400)]
    assert depth.regions("TANDUP", ["c", 1, 900], 900) == [(0, 0, 900, 900)]                      # both flanks empty
    assert depth.regions("DEL", ["c", 5000, 5400], 5200) == [(3999, 4999, 5200, 5200)]            # the event itself runs past the contig
    assert depth.regions("DEL", ["c", 5000, 5400], 0) == [(0, 0, 0, 0)]                           # a contig the file does not have
    for t in ("INV", "INS", "BND", "DISDUP", "DEL_INV", "DUP_INV", "Other"):
        assert depth.regions(t, ["c", s, s + 500], n) == []
    for regs in (depth.regions("DEL", ["c", 2, 30000], 29000), depth.regions("DEL", ["c", 700, 900], 800)):
        for b in regs:
            assert 0 <= b[0] <= b[1] <= b[2] <= b[3]


def test_payload_and_fold():
    # two regions of a long event: inside = the two probes, flanks = one each
    regs = [(1000, 2000, 12000, 12000), (40000, 40000, 50000, 51000)]
    p = depth.payload("DEL", regs, [[7000, 30000, 0], [0, 50000, 9000]])
    assert p == [80000, 20000, 16000, 2000]
    assert depth.fold("DEL", p) == ["4.00", "8.00", "0.500", "1"] and depth.fold("TANDUP", p) == ["4.00", "8.00", "0.500", "0"]
    assert depth.payload("INV", regs, [[1, 2, 3]] * 2) is None and depth.payload("DEL", [], []) is None
    # the thresholds are compared as exact ratios: 0.7 and 1.3 themselves support nothing
    assert depth.fold("DEL", [7, 10, 10, 10])[2:] == ["0.700", "0"] and depth.fold("DEL", [6999, 10000, 10, 10])[2:] == ["0.700", "1"]
    assert depth.fold("TANDUP", [13, 10, 10, 10])[2:] == ["1.300", "0"] and depth.fold("TANDUP", [13001, 10000, 10, 10])[2:] == ["1.300", "1"]
    # which columns become '.'
    assert depth.fold("DEL", None) == ["."] * 4 and depth.fold("DEL", [0, 0, 50, 10]) == ["."] * 4
    assert depth.fold("DEL", [30, 10, 0, 0]) == ["3.00", ".", ".", "."]
    assert depth.fold("DEL", [30, 10, 0, 20]) == ["3.00", "0.00", ".", "."]
    # products in integers: sums near 2^53 still give the exact verdict
    big = 1 << 52
    assert depth.fold("TANDUP", [13 * big + 1, 10, 10 * big, 10])[3] == "1" and depth.fold("TANDUP", [13 * big, 10, 10 * big, 10])[3] == "0"


# ------------------------------------------------------------------------------------------------------------------------------
# depth.cover against a per-base pile-up
# ------------------------------------------------------------------------------------------------------------------------------
COVERS, ADVANCES = {0, 7, 8}, {0, 2, 3, 7, 8}         # M = X; M D N = X


def pile(records, bounds, min_mapq=0, exclude=0):
    """The model: one increment per covered base, then slice sums.  records: (pos0, [(n, code)...], mapq, flag)."""
    b0, b1, b2, b3 = bounds
    d = np.zeros(b3 + 1, dtype=np.int64)
    for pos0, ops, mapq, flag in records:
        if mapq < min_mapq or flag & (exclude | 0x704):
            continue
        cur = pos0
        for n, code in ops:
            if code in COVERS:
                d[min(cur, b3):min(cur + n, b3)] += 1
            if code in ADVANCES:
                cur += n
    return [int(d[b0:b1].sum()), int(d[b1:b2].sum()), int(d[b2:b3].sum())]


def as_cover(records):
    return [(pos0 + 1, np.asarray([(n << 4) | c for n, c in ops], dtype=np.uint32)) for pos0, ops, _q, _f in records]


def test_cover_equals_the_pile_up_on_random_records():
    rng = np.random.default_rng(77)
    recs = []
    for _ in range(400):
        ops = [(int(rng.integers(0, 300)), int(rng.integers(0, 9))) for _ in range(int(rng.integers(0, 25)))]
        recs.append((int(rng.integers(0, 9000)), ops, 60, 0))
    assert {c for r in recs for _n, c in r[1]} == set(range(9))
    for bounds in ((2000, 3000, 5000, 6000), (0, 1, 2, 3), (4000, 4000, 4500, 4500), (100, 900, 900, 2500), (3000, 3000, 3000, 3000),
                   (0, 0, 0, 0), (0, 2500, 7000, 12000), (8999, 9000, 9001, 9002)):
        got = depth.cover(as_cover(recs), bounds)
        assert got == pile(recs, bounds), bounds
        assert all(isinstance(x, int) for x in got)
    assert depth.cover(as_cover(recs), (3000, 3000, 3000, 3000)) == [0, 0, 0]


def test_cover_on_designed_records():
    b = (1000, 2000, 3000, 4000)
    cases = {
        "one interval": [(1200, [(300, 0)], 60, 0)],
        "two intervals": [(1900, [(300, 7)], 60, 0)],
        "all three, one operation": [(500, [(4000, 8)], 60, 0)],
        "ends exactly at b0": [(700, [(300, 0)], 60, 0)],
        "starts exactly at b3": [(4000, [(300, 0)], 60, 0)],
        "one base into b0, one before b3": [(700, [(301, 0)], 60, 0), (3999, [(50, 0)], 60, 0)],
        "D and N inside an interval": [(1100, [(100, 0), (200, 2), (100, 0), (300, 3), (1500, 0)], 60, 0)],
        "I S H P do not move the cursor": [(1500, [(20, 4), (10, 5), (100, 0), (50, 1), (7, 6), (100, 0), (30, 4)], 60, 0)],
        "no operation": [(1500, [], 60, 0)],
        "zero-length operations": [(1500, [(0, 0), (0, 2), (10, 0)], 60, 0)],
    }
    want = {"one interval": [300, 0, 0], "two intervals": [100, 200, 0], "all three, one operation": [1000, 1000, 1000],
            "ends exactly at b0": [0, 0, 0], "starts exactly at b3": [0, 0, 0], "one base into b0, one before b3": [1, 0, 1],
            "D and N inside an interval": [400, 1000, 300], "I S H P do not move the cursor": [200, 0, 0], "no operation": [0, 0, 0],
            "zero-length operations": [10, 0, 0]}
    for name, recs in cases.items():
        assert depth.cover(as_cover(recs), b) == pile(recs, b) == want[name], name
    # empty intervals take nothing, their neighbours everything
    everything = [(0, [(5000, 0)], 60, 0)]
    assert depth.cover(as_cover(everything), (1000, 1000, 3000, 3000)) == [0, 2000, 0]
    assert depth.cover(as_cover(everything), (1000, 2000, 2000, 2600)) == [1000, 0, 600]
    assert depth.parse_cigar("3S10M2I4D5N6=7X8H1P") == [(3 << 4) | 4, (10 << 4), (2 << 4) | 1, (4 << 4) | 2, (5 << 4) | 3, (6 << 4) | 7, (7 << 4) | 8, (8 << 4) | 5, (1 << 4) | 6]
    assert depth.parse_cigar("*") == [] and depth.parse_cigar("") == []


# ------------------------------------------------------------------------------------------------------------------------------
# the native host reader
# ------------------------------------------------------------------------------------------------------------------------------
CODES = "MIDNSHP=X"
REFS = [("c", 90000), ("e", 5000), ("f", 20000)]
Q = 20


def _cigar(ops):
    return "".join("%d%s" % (n, CODES[c]) for n, c in ops) or "*"


def _seq_len(ops):
    return sum(n for n, c in ops if c in (0, 1, 4, 7, 8))


@pytest.fixture(scope="module")
def designed(tmp_path_factory):
    """A file of designed records on contig c (block size 8192), a contig without records, a contig with a few; the records as
    the model takes them, per contig."""
    rng = np.random.default_rng(9)
    rows = []           # (name, tid, pos0, ops, mapq, flag)
    for i, flag in enumerate((0x4, 0x100, 0x200, 0x400, 0x800, 0x10, 0x1, 0x904)):
        rows.append(("flag%x" % flag, 0, 10000 + 10 * i, [(1500, 0)], 60, flag))
    rows.append(("q_below", 0, 10200, [(1500, 0)], Q - 1, 0))
    rows.append(("q_at", 0, 10210, [(1500, 0)], Q, 0))
    rows.append(("no_cigar", 0, 10300, [], 60, 0))
    rows.append(("long_cg", 0, 9000, [(1, 0) if j % 2 == 0 else (1, 1) for j in range(70000)], 60, 0))
    rows.append(("dn", 0, 9500, [(40, 4), (300, 0), (700, 2), (25, 1), (400, 7), (900, 3), (500, 8), (30, 4)], 60, 0))
    for i in range(120):
        ops = [(int(rng.integers(1, 400)), int(rng.integers(0, 9))) for _ in range(int(rng.integers(1, 12)))]
        rows.append(("r%d" % i, 0, int(rng.integers(7000, 15000)), ops, int(rng.integers(0, 61)), int(rng.choice([0, 0, 0, 16, 0x800, 0x400, 0x100]))))
    for i in range(6):
        rows.append(("f%d" % i, 2, 3000 + 700 * i, [(1000, 0)], 60, 0))
    recs = []
    for name, tid, pos0, ops, mapq, flag in rows:
        n = _seq_len(ops)
        recs.append((name, tid, pos0, _cigar(ops), "ACGT" * (n // 4) + "ACGT"[:n % 4], None, mapq, flag))
    d = tmp_path_factory.mktemp("depth_files")
    path = str(d / "designed.bam")
    bamio.write_bam(path, REFS, recs, block_size=8192)
    by_tid = {t: [(r[2], r[3], r[4], r[5]) for r in rows if r[1] == t] for t in range(3)}
    return path, by_tid


BOUNDS = [(9000, 10000, 11000, 12000), (0, 9000, 9001, 90000), (10000, 10000, 11700, 11700), (10300, 10300, 10300, 10300),
          (7000, 9500, 12126, 16000), (11510, 11515, 11520, 11525), (0, 0, 0, 0)]


def _python_statement(path, chrom, bounds, flt=(0, 0)):
    b = bamio.BamFile(path)
    b.set_filter(*flt)
    recs = [(r[1], r[2]) for r in b.fetch_raw(chrom, bounds[0] + 1, bounds[3], exclude_more=depth.EXCLUDE)] if bounds[3] > bounds[0] else []
    return depth.cover(recs, bounds)


@pytest.mark.parametrize("flt", [(0, 0), (0, 0x800), (Q, 0), (Q, 0x810)])
def test_native_depth_equals_the_statement_and_the_pile_up(designed, flt, monkeypatch):
    path, by_tid = designed
    monkeypatch.setenv("VAPOR_BAM_DEVICE", "0")
    be = seqio.InProcessBam()
    be.read_filter = flt
    chroms = ["c"] * len(BOUNDS) + ["e", "f", "nowhere"]
    bounds = BOUNDS + [(0, 1000, 2000, 5000), (2000, 3000, 5000, 9000), (0, 10, 20, 30)]
    got = be.depth_many(None, path, chroms, bounds)
    for chrom, b, g in zip(chroms, bounds, got):
        tid = {"c": 0, "e": 1, "f": 2}.get(chrom)
        want = pile(by_tid[tid], b, *flt) if tid is not None else [0, 0, 0]
        assert g == want == _python_statement(path, chrom, b, flt), (chrom, b)
    assert got[len(BOUNDS)] == [0, 0, 0] and got[-1] == [0, 0, 0] and sum(got[len(BOUNDS) + 1]) > 0
    # the Python route of depth_many (VAPOR_BAM_NATIVE=0, or a library without the entries) gives the same
    monkeypatch.setenv("VAPOR_BAM_NATIVE", "0")
    assert be.depth_many(None, path, chroms, bounds) == got
    monkeypatch.delenv("VAPOR_BAM_NATIVE")

    class Without:
        def __getattr__(self, name):
            if name in ("vapor_bam_depth", "vapor_bam_depth_device"):
                raise AttributeError(name)
            return getattr(L.load(), name)
    real = L.load()
    monkeypatch.setattr(L, "_lib", Without())
    called = []
    monkeypatch.setattr(bamio.BamFile, "depth_native", lambda self, *a, **k: called.append(a))
    assert seqio.InProcessBam.depth_many(be, None, path, chroms, bounds) == got and not called
    monkeypatch.setattr(L, "_lib", real)


def test_what_never_counts_and_what_the_user_decides(designed):
    """Each of 0x4, 0x100, 0x200, 0x400 is dropped without being asked; 0x800 counts unless excluded; MAPQ Q - 1 is dropped at
    --min-mapq Q and Q is kept; a record without CIGAR covers nothing; --dedup-qname changes nothing."""
    path, by_tid = designed
    b = bamio.BamFile(path)
    win = (10000, 10000, 10100, 10100)
    only = [r for r in by_tid[0] if r[1] == [(1500, 0)]]
    base = pile([r for r in by_tid[0] if r not in only], win)[1]
    tid = b.tid["c"]

    def inside(flt=(0, 0)):
        b.set_filter(*flt)
        return b.depth_native(tid, win)[1]
    # of the eight flag records 0x800, 0x10, 0x1 count (0x904 holds 0x100 and 0x4): the first base of each is at 10000 + 10 i
    per = {0x800: 100 - 40, 0x10: 100 - 50, 0x1: 100 - 60}
    assert pile(only, win)[1] == sum(per.values()) == 150
    assert inside() - base == 150
    base_no_supp = pile([r for r in by_tid[0] if r not in only], win, 0, 0x800)[1]
    assert inside((0, 0x800)) - base_no_supp == 150 - per[0x800]
    win2 = (10200, 10200, 10220, 10220)
    got = {q: None for q in (0, Q, Q + 1)}
    for q in got:
        b.set_filter(q, 0)
        got[q] = b.depth_native(tid, win2)[1] - pile([r for r in by_tid[0] if r[1] != [(1500, 0)] or r[2] == 60], win2, q, 0)[1]
    # q_below covers [10200, 10220): 20 bases, q_at [10210, 10220): 10 bases
    assert got == {0: 30, Q: 10, Q + 1: 0}
    b.set_filter(0, 0)
    want = b.depth_native(tid, BOUNDS[0])
    b.set_dedup(True)
    assert b.depth_native(tid, BOUNDS[0]) == want == pile(by_tid[0], BOUNDS[0])
    b.close()


def test_native_depth_refuses_bad_bounds(designed):
    path, _ = designed
    b = bamio.BamFile(path)
    for bad in ((-1, 0, 5, 9), (5, 4, 6, 9), (0, 5, 4, 9), (0, 5, 9, 8), (0, 5, 9, 1 << 31)):
        with pytest.raises(ValueError):
            b.depth_native(0, bad, [(b.first_record, b.first_record + 1)])
    with pytest.raises(ValueError):
        b.depth_native(-1, (0, 1, 2, 3), [(b.first_record, b.first_record + 1)])
    b.close()


def test_abi_surface():
    h = open(os.path.join(ROOT, "include", "vapor_hip.h")).read()
    for name in ("vapor_bam_depth", "vapor_bam_depth_device"):
        assert re.search(r"\bint %s\(" % name, h) and name in L.EXPORTS and name in L.OPTIONAL_EXPORTS and hasattr(L.load(), name)
    assert L.ABI_VERSION == 3


# ------------------------------------------------------------------------------------------------------------------------------
# tools/bam_check.cpp: the depth pass under the sanitizers
# ------------------------------------------------------------------------------------------------------------------------------
def test_depth_pass_under_sanitizers_on_good_and_damaged_files(designed, tmp_path):
    exe = str(tmp_path / "bam_check")
    cmd = ["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "vapor_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tools", "bam_check.cpp"), "-lz", "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(path, first, win, *more):
        p = subprocess.run([exe, path, str(first), "0", str(win[0]), str(win[1]), "200", "2"] + [str(m) for m in more], env=env,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, (path, p.returncode, p.stderr[-2000:])
        return p.stdout.splitlines()
    path, by_tid = designed
    first = bamio.BamFile(path).first_record
    # every record of the file walked: the sums are the pile-up's over [0, s) [s, e) [e, 2^31 - 1) - no record passes base 90 000
    for flt in ((), (Q, 0x800)):
        out = run(path, first, (10000, 11000), *flt, "depth")
        want = pile(by_tid[0], (0, 10000, 11000, REFS[0][1]), *(flt or (0, 0)))
        assert out[-1].split()[:6] == ["depth:", "rc", "0", "cov"] + [str(want[0]), str(want[1])], out[-1]
        assert int(out[-1].split()[6]) == want[2]
    # without the argument the program prints what it printed before
    assert not any(ln.startswith("depth:") for ln in run(path, first, (10000, 11000)))
    # the damaged files of tests/test_bamio.py: a status, never a report
    small = TB._small_bam(tmp_path)
    first = bamio.BamFile(small).first_record
    assert run(small, first, (4000, 5500), "depth")[-1].startswith("depth: rc 0 cov ")
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
        last = run(bad, first, (4000, 5500), "depth")[-1]
        assert last.startswith("depth: rc "), last
        n_err += last.startswith("depth: rc -4")
    assert n_err >= 7, n_err              # (a file cut between two blocks may end like one without EOF marker)


# ------------------------------------------------------------------------------------------------------------------------------
# the mode's surface (what tests/test_modes_cpu.py checks for the other three)
# ------------------------------------------------------------------------------------------------------------------------------
def test_payload_round_trip_and_columns():
    m = modes.DEPTH
    assert m.name == "depth" and m.pack(None) == [] and m.unpack(m.pack(None)) is None and m.unpack([]) is None
    for x in (depth.Payload([0, 600, 16000, 2000], "DEL"), depth.Payload([240000, 20000, 16000, 2000], "TANDUP"),
              depth.Payload([(1 << 53) - 1, 1, 0, 0], "TANDUP")):
        flat = m.pack(x)
        assert flat and all(isinstance(v, float) for v in flat)
        back = m.unpack(flat)
        assert type(back) is depth.Payload and list(back) == list(x) and back.svtype == x.svtype
        assert len(m.columns_many([x, None])[0]) == len(m.COLUMNS)
    assert len(m.COLUMNS) == len(m.INFO) == len(m.keys) == len(m.columns_many([None])[0]) == 4
    assert m.columns_many([None])[0] == ["."] * 4
    assert [i[0] for i in m.INFO] == list(m.COLUMNS) == ["VaPoR_DP_IN", "VaPoR_DP_FL", "VaPoR_DFC", "VaPoR_DSUP"]
    assert all(len(i) == 4 for i in m.INFO) and m.attr == "depth" and tuple(m.keys) == tuple(m.COLUMNS) and m.skip_dot and not m.phased
    assert m.columns_many([depth.Payload([240000, 20000, 16000, 2000], "TANDUP"), depth.Payload([240000, 20000, 16000, 2000], "DEL")]) == [
        ["12.00", "8.00", "1.500", "1"], ["12.00", "8.00", "1.500", "0"]]


def test_info_lines_and_record_keys_of_the_annotated_vcf(tmp_path):
    m = modes.DEPTH
    vcf = tmp_path / "in.vcf"
    vcf.write_text('##fileformat=VCFv4.1\n##INFO=<ID=SVTYPE,Number=1,Type=String,Description="t">\n##source=x\n'
                   "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
                   "c1\t100\ta\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=500\nc1\t900\tb\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=990\n")
    values = ["4.00", "8.00", "0.500", "1"]
    table = "\t".join(["#CHR"] * 10 + list(m.COLUMNS)) + "\n"
    table += "\t".join(["c1:100:500:DEL", "0.5", "0.25", "0/1", "1.5", "0.5,-1.0"] + values) + "\n"
    table += "\t".join(["c1:900:990:DEL", "0.5", "0.25", "0/1", "1.5", "0.5,-1.0"] + ["3.00", ".", ".", "."]) + "\n"
    (tmp_path / "in.vcf.vapor").write_text(table)
    SF.vcf_vapor_modify(str(vcf), {"c1:100:500:DEL": [4], "c1:900:990:DEL": [5]}, mode=m)
    with_mode = (tmp_path / "in.vcf.vapor").read_text().splitlines()
    (tmp_path / "in.vcf.vapor").write_text(table)
    SF.vcf_vapor_modify(str(vcf), {"c1:100:500:DEL": [4], "c1:900:990:DEL": [5]})
    plain = (tmp_path / "in.vcf.vapor").read_text().splitlines()
    new = [ln for ln in with_mode if ln not in plain and ln.startswith("##")]
    at = with_mode.index(new[0])
    assert with_mode[at - 1].startswith("##INFO=<ID=VaPoR_REC,") and with_mode[at:at + len(new)] == new
    got = [re.fullmatch(r'##INFO=<ID=(\w+),Number=([1.]),Type=(\w+),Description="([^"]+)">', ln).groups() for ln in new]
    assert [g[0] for g in got] == list(m.COLUMNS) and all(g[1] == "1" for g in got)
    assert [g[2] for g in got] == ["Float", "Float", "Float", "Integer"]
    assert all(g[3].endswith("(--depth)") for g in got)
    recs = [ln.split("\t") for ln in with_mode if not ln.startswith("#")]
    recs_plain = [ln.split("\t") for ln in plain if not ln.startswith("#")]
    assert len(recs) == 2 and [r[7] for r in recs_plain] == [r[7].split(";" + m.keys[0] + "=")[0] for r in recs]
    assert recs[0][7][len(recs_plain[0][7]):] == "".join(";%s=%s" % kv for kv in zip(m.keys, values))
    assert recs[1][7][len(recs_plain[1][7]):] == ";VaPoR_DP_IN=3.00"                  # the '.' keys are left out


# ------------------------------------------------------------------------------------------------------------------------------
# cli.main on a world whose depth is known
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def fake(oracle):
    pipeline.set_engine(FakeEngine(oracle))
    yield
    pipeline.set_engine(None)
    seqio.set_backend(None)


def _main(tmp_path, name, mode, text, more=()):
    d = tmp_path / name
    d.mkdir()
    src = d / ("in." + mode)
    src.write_text(text)
    out = d / "out.vapor"
    args = [mode, "--sv-input", str(src), "--reference", "ref.fa", "--pacbio-input", "x.bam", "--output-path", str(d / "figs"),
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
    return [r.split("\t") for r in table.splitlines()], annotated


LAYERS = 4
# Error-free reads, `LAYERS` layers a haplotype: every base of a haplotype lies in exactly LAYERS reads (make_depth_world), so
# outside an event the depth is 2 * LAYERS = 8.  Inside: a het DEL keeps the reference haplotype's LAYERS = 4; a hom DEL has
# none; a het TANDUP has the reference haplotype's 4 and twice the alt haplotype's 4 = 12, so DFC = 12 / 8 = 1.5; a hom TANDUP
# 2 * 2 * 4 = 16.  A D, a soft clip and a 0x800 piece cover what the text says, so none of this depends on where a read was cut.
EXPECT = [("DEL", "hom", ["0.00", "8.00", "0.000", "1"]), ("DEL", "het", ["4.00", "8.00", "0.500", "1"]),
          ("TANDUP", "het", ["12.00", "8.00", "1.500", "1"]), ("TANDUP", "hom", ["16.00", "8.00", "2.000", "1"]),
          ("INV", "het", [".", ".", ".", "."]), ("DEL", "het", ["4.00", "8.00", "0.500", "1"]),
          ("TANDUP", "het", ["12.00", "8.00", "1.500", "1"])]


def test_cli_on_a_depth_world_in_memory(fake, tmp_path):
    w = synth.make_depth_world(seed=4, layers=LAYERS)
    assert [(l.svtype, z) for l, (_t, _n, z) in zip(w.loci, synth.DEPTH_SPECS)] == [e[:2] for e in EXPECT]
    assert any(l.end - l.start + 1 > 2 * P for l in w.loci) and any(r.flag == 0x800 for rs in w.reads.values() for r in rs)
    assert any("D" in r.cigar for rs in w.reads.values() for r in rs) and any("S" in r.cigar for rs in w.reads.values() for r in rs)
    text = synth.bed_text(w)
    seqio.set_backend(seqio.MemorySamtools(w))
    plain, _ = _main(tmp_path, "plain", "bed", text)
    seqio.set_backend(seqio.MemorySamtools(w))
    rows, _ = _main(tmp_path, "depth", "bed", text, ["--depth"])
    assert rows[0][-4:] == list(depth.COLUMNS) and rows[0][:-4] == plain[0]
    assert len(rows) == len(plain) == len(w.loci) + 1
    for r, p, e in zip(rows[1:], plain[1:], EXPECT):
        assert r[:-4] == p, e                      # the row's own columns, byte for byte
        assert r[-4:] == e[2], (e, r[-4:])
    # the other options it goes with leave the plain columns of their own runs alone, and 0x800 excluded changes the numbers
    seqio.set_backend(seqio.MemorySamtools(w))
    flt_plain, _ = _main(tmp_path, "flt_plain", "bed", text, ["--exclude-flags", "0x800", "--dedup-qname"])
    seqio.set_backend(seqio.MemorySamtools(w))
    flt, _ = _main(tmp_path, "flt", "bed", text, ["--depth", "--exclude-flags", "0x800", "--dedup-qname"])
    assert [r[:-4] for r in flt[1:]] == flt_plain[1:]
    assert flt[1][-4:] == EXPECT[0][2] and flt[3][-4:] != EXPECT[2][2]          # (the second copy's clipped pieces are 0x800 records)
    # vcf: DEL records get the INFO keys, an INV record none; TANDUP is not scored by `vapor vcf`
    vtext = synth.vcf_text(w)
    seqio.set_backend(seqio.MemorySamtools(w))
    vplain, _ = _main(tmp_path, "vplain", "vcf", vtext)
    seqio.set_backend(seqio.MemorySamtools(w))
    vrows, annotated = _main(tmp_path, "vdepth", "vcf", vtext, ["--depth"])
    assert [r[:-4] for r in vrows] == vplain
    by_key = {r[0]: r[-4:] for r in vrows[1:]}
    for l, e in zip(w.loci, EXPECT):
        if l.svtype in ("DEL", "INV"):
            assert by_key["%s:%d:%d:%s" % (l.chrom, l.start, l.end, l.svtype)] == e[2]
    lines = annotated.splitlines()
    assert sum(ln.startswith("##INFO=<ID=VaPoR_D") for ln in lines) == 4
    rec = {ln.split("\t")[2]: ln.split("\t")[7] for ln in lines if not ln.startswith("#")}
    assert rec["dp1"].endswith(";VaPoR_DP_IN=0.00;VaPoR_DP_FL=8.00;VaPoR_DFC=0.000;VaPoR_DSUP=1")
    assert rec["dp6"].endswith(";VaPoR_DP_IN=4.00;VaPoR_DP_FL=8.00;VaPoR_DFC=0.500;VaPoR_DSUP=1")
    assert "VaPoR_DP_IN" not in rec["dp5"] and "VaPoR_DSUP" not in rec["dp5"]


def test_the_sam_text_backends_take_column_six(tmp_path):
    """SamtoolsCLI / SamtoolsHybrid: POS and CIGAR of `view`'s lines behind _sam_fields' filter, lengths from the .fai."""
    w = synth.make_depth_world(seed=5, specs=(("DEL", 700, "het"), ("TANDUP", 24000, "het")), errors=(0.01, 0.02, 0.02))
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
            assert n == mem.contig_length("x", "r", l.chrom) == len(w.contigs[l.chrom])
            regs = depth.regions(l.svtype, [l.chrom, l.start, l.end], n)
            assert len(regs) == (2 if l.end - l.start + 1 > 2 * P else 1)
            got = txt.depth_many(None, "x", [l.chrom] * len(regs), regs)
            assert got == mem.depth_many(None, "x", [l.chrom] * len(regs), regs) and sum(got[0]) > 0

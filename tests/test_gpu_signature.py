"""Split-read and CIGAR evidence on the device (`--signatures`, DESIGN.md 4.20: vapor_bam_signature_device - bgzf_inflate_kernel,
bam_signature_kernel) against the native host reader (vapor_bam_signature), the Python statement (signature.answer over bamio's
records) and the brute force of tests/test_signature_cpu.py: per region the ten words and the status, exactly - one region per way
the kernel can go wrong, 300 regions in one call and split over many, a file with a damaged block (a handled status), and the
CLI's tables from files."""
import shutil

import numpy as np
import pytest

import test_bamio as TB
import test_gpu_depth as GD
import test_signature_cpu as SC
from vapor_amd import _lib as L
from vapor_amd import bamio, pipeline, seqio, signature, synth
from vapor_amd.engine import Engine

pytestmark = pytest.mark.gpu

REG_BLOCK = 5
C, T = SC.C, SC.T
NCAP = SC.NCAP
M, I, D, N, S, H, PAD, EQ, X = range(9)
LC0, RC0, LC1, RC1, GAP, INSOP = 1, 2, 4, 8, 16, 32


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def device(eng, b, chroms, regions):
    """engine.bam_signature_device over the regions' .bai chunks: (ten words per region, status per region, chunks per region)."""
    tids = [b.tid[c] for c in chroms]
    chunk_first, flat, per = [0], [], []
    for t, rg in zip(tids, regions):
        ch = b.index.chunks(t, int(rg[0]), int(rg[1])) if rg[1] > rg[0] else []
        per.append(ch)
        for c in ch:
            flat += [c[0], c[1]]
        chunk_first.append(len(flat) // 2)
    with b.handle(L.load()) as tl:
        out, status = eng.bam_signature_device(tl["native"], tids, np.asarray(regions, dtype=np.int64).reshape(-1, 9), chunk_first,
                                               np.asarray(flat, dtype=np.uint64))
    return [[int(x) for x in o] for o in out], status.tolist(), per


def statement(b, chrom, rg):
    recs = [(r[1], r[2]) for r in b.fetch_raw(chrom, int(rg[0]) + 1, int(rg[1]), exclude_more=signature.EXCLUDE)] if rg[1] > rg[0] else []
    return signature.words(signature.answer(recs, rg))


# ------------------------------------------------------------------------------------------------------------------------------
# one region per way the kernel can go wrong
# ------------------------------------------------------------------------------------------------------------------------------
PATTERN = [(3, M), (2, D), (1, I), (4, X), (5, N), (2, EQ), (6, PAD)]        # the cursor moves by 16 every seven operations
N_OPS = (0, 1, 2, 3, 63, 64, 65, 66, 128, 129, 4000)
BLOCK = 4096
X0, X1 = 20000, 20600            # the breakpoints of contig `rule`
OFFS = (-T - 1, -T, 0, T, T + 1)
MODES = [([], [0, 0]), ([17], [17, 1]), ([-60], [-60, 1]), ([60], [60, 1]), ([3, 3, -9, -9, -9, 20], [-9, 3]), ([5, 5, -2, -2, 30, 30], [-2, 2]),
         ([4, -4], [-4, 1]), ([-4, 4, 4, -4], [-4, 2]), ([0, 1, -1], [0, 1]), ([1, -1, 2, -2], [-1, 1]), ([60, -60, 59], [59, 1])]


def ops_of(n):
    """A record of n operations: a leading 40S, the pattern, and the last two operations a 20S and a 15H that reach C only
    together - at n = 65 and n = 129 the two lie in two different tiles."""
    if n <= 3:
        return [[], [(200, M)], [(40, S), (200, M)], [(40, S), (200, M), (35, S)]][n]
    return [(40, S)] + [PATTERN[i % len(PATTERN)] for i in range(n - 3)] + [(20, S), (15, H)]


def span_of(ops):
    return sum(n for n, c in ops if c in SC.ADVANCES)


@pytest.fixture(scope="module")
def designed(tmp_path_factory):
    rows = []                                        # (name, tid, pos0, ops, mapq, flag)
    refs = [("ops", 80000), ("edge", 40000), ("cg", 120000), ("rule", 40000), ("mode", 200000), ("two", 140000), ("flt", 50000), ("none", 9000)]
    for k, n in enumerate(N_OPS):
        rows.append(("n%d" % n, 0, 5000 * k + 100, ops_of(n), 60, 0))
        rows.append(("m%d" % n, 0, 5000 * k + 130, [(45, H), (900, M)], 60, 0))           # a neighbour in the same window
    # the trailing clip as operation 63, 64 and 65 (one S of C bases: lane 63 of the first tile, lanes 0 and 1 of the second)
    for k, n in enumerate((64, 65, 66)):
        rows.append(("t%d" % n, 1, 1000 + 2000 * k, [((1, M), (1, EQ))[i % 2] for i in range(n - 1)] + [(C, S)], 60, 0))
    # a GAP on lane 63 and an INSOP on lane 0 of the next tile, and the other way round: the cursor is carried over the tile edge
    fill = [((1, M), (1, X))[i % 2] for i in range(63)]
    rows.append(("gap63", 1, 10000, fill + [(600, D), (40, I), (100, M)], 60, 0))
    rows.append(("ins63", 1, 20000, fill + [(40, I), (600, D), (100, M)], 60, 0))
    rows.append(("gap127", 1, 30000, fill + [(1, EQ)] + fill + [(600, N), (40, I), (100, M)], 60, 0))
    # CG:B,I: 70 000 operations that reach 60 000 with a GAP of 800 and a trailing clip behind it
    rows.append(("cg", 2, 60000 - 34998, [(1, M) if j % 2 == 0 else (1, I) for j in range(69996)] + [(800, D), (0, M), (33, S), (9, H)], 60, 0))
    rows.append(("cg_after", 2, 95000, [(40, S), (400, M)], 60, 0))
    # the rule at its edges, on contig `rule`: every bit at the offsets -T - 1 .. T + 1, the length bounds, the clip sums
    for off in OFFS:
        rows.append(("l0_%d" % off, 3, X0 + off, [(40, S), (100, M)], 60, 0))
        rows.append(("r0_%d" % off, 3, X0 + off - 100, [(100, M), (40, S)], 60, 0))
        rows.append(("l1_%d" % off, 3, X1 + off, [(40, H), (100, M)], 60, 0))
        rows.append(("r1_%d" % off, 3, X1 + off - 100, [(100, M), (40, H)], 60, 0))
        rows.append(("g_%d" % off, 3, X0 + off - 100, [(100, M), (600, D), (100, M)], 60, 0))
        rows.append(("i0_%d" % off, 3, X0 + off - 100, [(100, M), (400, I), (100, M)], 60, 0))
        rows.append(("i1_%d" % off, 3, X1 + off - 100, [(100, M), (400, I), (100, M)], 60, 0))
    for n in (579, 580, 620, 621):
        rows.append(("gn_%d" % n, 3, X0 - 90, [(100, M), (n, D), (100, M)], 60, 0))
        rows.append(("in_%d" % n, 3, X0 - 80, [(100, M), (n, I), (100, M)], 60, 0))
    rows.append(("c_below", 3, X0 + 7, [(C - 1, S), (100, M)], 60, 0))
    rows.append(("c_at", 3, X0 + 8, [(C, S), (100, M)], 60, 0))
    rows.append(("hs_below", 3, X0 + 9, [(C - 10, H), (9, S), (100, M)], 60, 0))
    rows.append(("hs_at", 3, X0 + 10, [(C - 10, H), (10, S), (100, M)], 60, 0))
    rows.append(("all_clip", 3, X0, [(100, H), (100, S)], 60, 0))
    # the modes: one locus per list of offsets, 10 000 bases apart
    for k, (offs, _want) in enumerate(MODES):
        for j, o in enumerate(offs):
            rows.append(("mo%d_%d" % (k, j), 4, 10000 * (k + 1) + o, [(40, S), (200, M)], 60, 0))
    # two .bai chunks: a long record in a high bin, records of another leaf bin behind it in the file, then the window's own
    rows.append(("long", 5, 10000, [(35000, M), (40, S)], 60, 0))
    for i in range(40):
        rows.append(("gap%d" % i, 5, 12000 + 10 * i, [(300, M)], 60, 0))
    for i in range(12):
        rows.append(("own%d" % i, 5, 39000 + 150 * i, [(35, S), (500, M), (40, D), (500, EQ), (35, S)], 60, 0))
    rows.append(("ends_at_w0", 5, 39440, [(500, M), (40, S)], 60, 0))
    rows.append(("at_w3", 5, 41000, [(40, S), (700, M)], 60, 0))
    rows.append(("behind_w3", 5, 41500, [(40, S), (700, M)], 60, 0))
    # filtered records first, three in a row, last; and a stretch where every record is filtered
    for i, flag in enumerate((0x4, 0, 0, 0x100, 0x200, 0x400, 0, 0x800, 0, 0x400)):
        rows.append(("f%d" % i, 6, 2000 + 3 * i, [(40, S), (1000, M)], 60, flag))
    for i in range(5):
        rows.append(("all%d" % i, 6, 30000 + 5 * i, [(40, S), (600, M)], 60, (0x100, 0x400, 0x4, 0x200, 0x704)[i]))
    path = str(tmp_path_factory.mktemp("gpu_signature") / "designed.bam")
    SC.write_rows(path, refs, rows, block_size=BLOCK)
    # a record header across two BGZF blocks, by design: the file again with a block size that puts a block boundary 18 bytes
    # behind the start of the 4000-operation record (where a record starts in the inflated stream does not depend on the blocks)
    q = [q for q, name in GD._record_starts(path) if name == "n4000"][0]
    k = max(1, round(q / BLOCK))
    block = (q + 18) // k
    SC.write_rows(path, refs, rows, block_size=block)
    by_chrom = {name: [(r[2], r[3], r[4], r[5]) for r in rows if r[1] == t] for t, (name, _n) in enumerate(refs)}
    return path, by_chrom, block


def around(x0, x1, tol=T, mc=C, nmin=0, nmax=NCAP, mask=63):
    return (max(min(x0, x1) - tol - 1, 0), max(x0, x1) + tol + 1, x0, x1, tol, mc, nmin, nmax, mask)


def _cases():
    out = []
    for k, n in enumerate(N_OPS):
        pos = 5000 * k + 100
        out.append(("%d operations" % n, "ops", around(pos, pos + span_of(ops_of(n)), nmin=1, nmax=10)))
    for k, n in enumerate((64, 65, 66)):
        pos = 1000 + 2000 * k
        out.append(("the trailing clip as operation %d" % (n - 1), "edge", around(pos, pos + n - 1, mask=RC1)))
    out += [
        ("GAP on lane 63, INSOP on lane 0", "edge", around(10063, 10663, nmin=30, nmax=700)),
        ("INSOP on lane 63, GAP on lane 0", "edge", around(20063, 20663, nmin=30, nmax=700)),
        ("GAP on lane 63 of the second tile", "edge", around(30127, 30727, nmin=30, nmax=700)),
        ("CG:B,I of 70 000 operations", "cg", around(60000, 60800, nmin=400, nmax=1600)),
        ("CG:B,I, its I operations", "cg", around(59990, 60000, tol=5, nmin=1, nmax=1, mask=INSOP)),
        ("every bit, every offset", "rule", around(X0, X1, nmin=300, nmax=1200)),
        ("tol 0", "rule", around(X0, X1, tol=0, nmin=300, nmax=1200)),
        ("tol 255", "rule", around(X0, X1, tol=255, nmin=300, nmax=1200)),
        ("tol T - 1", "rule", around(X0, X1, tol=T - 1, nmin=300, nmax=1200)),
        ("x0 == x1", "rule", around(X0, X0, nmin=300, nmax=1200)),
        ("x0 == x1 at the right breakpoint", "rule", around(X1, X1, nmin=0, nmax=0, mask=LC0 | RC0)),
        ("n from nmin to nmax", "rule", around(X0, X1, nmin=580, nmax=620)),
        ("min_clip 1", "rule", around(X0, X1, mc=1, nmin=0, nmax=0)),
        ("min_clip C + 11", "rule", around(X0, X1, mc=C + 11, nmin=0, nmax=0)),
        ("all bits off", "rule", around(X0, X1, nmin=300, nmax=1200, mask=0)),
    ]
    out += [("bit %d alone" % bit, "rule", around(X0, X1, nmin=300, nmax=1200, mask=1 << bit)) for bit in range(6)]
    out += [("mode of %r" % (offs,), "mode", (10000 * (k + 1) - 100, 10000 * (k + 1) + 100, 10000 * (k + 1), 10000 * (k + 1) + 5000, 60, C, 0, 0, LC0))
            for k, (offs, _w) in enumerate(MODES)]
    out += [
        ("two .bai chunks; before w0, at w3, behind w3", "two", (39940, 41000, 39991, 41000, T, C, 30, 50, 63)),
        ("a clip of a long record in a high bin", "two", around(45000, 45000, mask=RC0)),
        ("filtered first, three in a row, last", "flt", around(2010, 2010, mask=LC0)),
        ("all filtered", "flt", around(30010, 30010, mask=LC0)),
        ("a contig without records", "none", around(1000, 2000)),
        ("an empty window", "two", (40000, 40000, 39990, 39990, T, C, 0, 0, 63)),
        ("w0 = 0", "ops", (0, 200, 100, 100, T, C, 0, 0, 63)),
    ]
    return out


def test_every_designed_region_equals_host_statement_and_model(eng, designed):
    path, by_chrom, block = designed
    b = bamio.BamFile(path)
    cases = _cases()
    chroms, regions = [c[1] for c in cases], [c[2] for c in cases]
    out, status, chunks = device(eng, b, chroms, regions)
    assert status == [0] * len(cases), status
    for (name, chrom, rg), got in zip(cases, out):
        host = b.signature_native(b.tid[chrom], rg)
        want = SC.brute(by_chrom[chrom], rg)
        assert got == host == want == statement(b, chrom, rg), (name, got, host, want)
    by_name = {c[0]: (g, ch) for c, g, ch in zip(cases, out, chunks)}
    # the properties the cases are there for
    for n in N_OPS:
        got = by_name["%d operations" % n][0]
        # the record's own clips (the neighbour adds a leading one): none without CIGAR, none for a single M, a leading one from 2 on,
        # a trailing one from 3 on - as 20S + 15H, in two tiles at 65 and 129
        assert got[0] == (2 if n >= 2 else 1) and got[3] == (1 if n >= 3 else 0), (n, got)
        assert got[5] == len([1 for i in range(max(n - 3, 0)) if PATTERN[i % 7][1] == I]) and (n < 100 or got[5] > 10)
    assert all(by_name["the trailing clip as operation %d" % k][0][:6] == [0, 0, 0, 1, 0, 0] for k in (63, 64, 65))
    # (an I behind the D lies at x1, out of the left histogram's reach; one before it lies at x0 with the D)
    for name, at_x0 in (("GAP on lane 63, INSOP on lane 0", 1), ("INSOP on lane 63, GAP on lane 0", 2), ("GAP on lane 63 of the second tile", 1)):
        assert by_name[name][0] == [0, 0, 0, 0, 1, 1, 0, at_x0, 0, 1], (name, by_name[name][0])
    assert by_name["CG:B,I of 70 000 operations"][0] == [0, 0, 0, 1, 1, 0, 0, 1, 0, 2]
    assert by_name["CG:B,I, its I operations"][0][5] == 16         # one I behind every M: those at the cursors 59 985 .. 60 000
    every = by_name["every bit, every offset"][0]
    assert every[:4] == [3 + 2, 3, 3, 3] and every[4] == 3 + 4 and every[5] == 2 * 5 - 2 + 4      # three of five offsets; c_at and hs_at; the length cases
    assert by_name["tol 0"][0][:4] == [1, 1, 1, 1] and by_name["tol T - 1"][0][1:4] == [1, 1, 1] and by_name["tol 255"][0][1:4] == [5, 5, 5]
    assert by_name["n from nmin to nmax"][0][4:6] == [3 + 2, 2] and by_name["all bits off"][0] == [0] * 10
    assert by_name["min_clip 1"][0][0] == 3 + 4 and by_name["min_clip C + 11"][0][:4] == [0, 0, 0, 0]
    for bit in range(6):
        got = by_name["bit %d alone" % bit][0]
        assert got[bit] == every[bit] and sum(got[:6]) == every[bit]
    both = by_name["x0 == x1"][0]
    assert both[0] == both[2] == every[0] and both[1] == both[3] == every[1] and both[4] == 0
    for offs, want in MODES:
        got = by_name["mode of %r" % (offs,)][0]
        assert got[6:8] == want and got[0] == len(offs) and got[8:] == [0, 0], (offs, got)
    two = by_name["two .bai chunks; before w0, at w3, behind w3"]
    assert len(two[1]) == 2 and two[0][:6] == [0, 1, 0, 0, 0, 0] and two[0][6:8] == [49, 1]      # the clip at w3 = x1 is not met
    assert by_name["a clip of a long record in a high bin"][0][:6] == [0, 1, 0, 0, 0, 0]
    assert by_name["filtered first, three in a row, last"][0][0] == 5 and by_name["all filtered"][0] == [0] * 10
    assert by_name["a contig without records"][0] == [0] * 10 and by_name["an empty window"][0] == [0] * 10
    assert by_name["an empty window"][1] == [] and by_name["w0 = 0"][0][0] == 1
    # a record header across two BGZF blocks is among the records walked: the 4000-operation record's
    starts = dict((name, q) for q, name in GD._record_starts(path))
    assert starts["n4000"] // block + 1 == (starts["n4000"] + 35) // block
    b.close()


def test_with_the_handles_filter(eng, designed):
    path, by_chrom, _block = designed
    b = bamio.BamFile(path)
    rg = around(2010, 2010, mask=LC0)
    seen = []
    for flt in ((0, 0), (0, 0x800), (61, 0), (60, 0x800)):
        b.set_filter(*flt)
        out, status, _ = device(eng, b, ["flt", "rule"], [rg, around(X0, X1, nmin=300, nmax=1200)])
        assert status == [0, 0]
        assert out[0] == b.signature_native(b.tid["flt"], rg) == SC.brute(by_chrom["flt"], rg, *flt) == statement(b, "flt", rg)
        seen.append(out[0][0])
    assert seen == [5, 4, 0, 4]
    b.set_filter(0, 0)
    b.set_dedup(True)
    assert device(eng, b, ["flt"], [rg])[0][0][0] == 5                   # --dedup-qname has no effect
    b.close()


def test_refused_regions_and_arguments(eng, designed):
    path, _, _block = designed
    b = bamio.BamFile(path)
    with b.handle(L.load()) as tl:
        ch = np.asarray(b.index.chunks(0, 0, 5000), dtype=np.uint64).reshape(-1)
        good = (0, 300, 100, 100, T, C, 0, 10, 63)
        bad = [good[:k] + (v,) + good[k + 1:] for k, v in ((0, 301), (1, 1 << 31), (4, -1), (4, 256), (6, 11), (0, -1))]
        regions = np.asarray([good] + bad + [good], dtype=np.int64)
        n = len(regions)
        first = np.arange(n + 1, dtype=np.int32) * (len(ch) // 2)
        out, status = eng.bam_signature_device(tl["native"], [0] * (n - 1) + [-1], regions, first, np.tile(ch, n))
        assert status.tolist() == [0] + [2] * (n - 1) and out[1:].tolist() == [[0] * 10] * (n - 1) and out[0].tolist() == b.signature_native(0, good)
        assert out[0][0] == 1
        out, status = eng.bam_signature_device(tl["native"], [], np.zeros((0, 9), dtype=np.int64), [0], [])
        assert len(out) == 0 and len(status) == 0
    b.close()


# ------------------------------------------------------------------------------------------------------------------------------
# many regions
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many(tmp_path_factory):
    rng = np.random.default_rng(12)
    n = 60000
    rows = [("m%d" % i, 0) + r for i, r in enumerate(SC.seeded_records(rng, 2500, 0, n - 3000, clip_p=0.8))]
    path = str(tmp_path_factory.mktemp("gpu_signature_many") / "many.bam")
    SC.write_rows(path, [("c", n)], rows, block_size=20000)
    regions = []
    for _ in range(300):
        x0 = int(rng.integers(300, n - 3000))
        x1 = x0 + int(rng.integers(0, 130))
        tol = int(rng.choice([0, 5, T, 120, 255]))
        nmin = int(rng.integers(0, 60))
        regions.append((max(x0 - tol - 1, 0), x1 + tol + 1, x0, x1, tol, int(rng.integers(1, 45)), nmin, nmin + int(rng.integers(0, 120)), int(rng.integers(0, 64))))
    return path, regions, [r[2:] for r in rows]


def test_300_regions_in_one_call_and_split_and_halved(eng, many, monkeypatch):
    path, regions, recs = many
    b = bamio.BamFile(path)
    out, status, chunks = device(eng, b, ["c"] * 300, regions)
    assert status == [0] * 300
    host = [b.signature_native(0, rg) for rg in regions]
    assert out == host
    for g in range(0, 300, 10):
        assert out[g] == statement(b, "c", regions[g]) == SC.brute(recs, regions[g])
    assert sum(sum(o[:6]) > 0 for o in out) > 100 and sum(o[7] > 1 for o in out) > 10
    b.close()
    # the same through signature_many, its groups so small that the call is split, and a library that refuses more than 8 regions
    # "in one call" so that the groups are halved
    calls = []

    class Refusing:
        def bam_signature_device(self, native, tids, *a):
            calls.append(len(tids))
            if len(tids) > 8:
                raise L.VaporHipError(-4, "vapor_bam_signature_device: more than 1.5 GB of blocks in one call (use smaller batches)")
            return eng.bam_signature_device(native, tids, *a)
    monkeypatch.setenv("VAPOR_BAM_DEVICE_BATCH_MB", "8")
    be = seqio.InProcessBam()
    assert be.signature_many(Refusing(), path, ["c"] * 300, regions) == host
    big, small = [c for c in calls if c > 8], [c for c in calls if c <= 8]
    assert len(big) >= 3 and sum(small) == 300 and max(calls) < 300
    calls.clear()
    monkeypatch.setenv("VAPOR_BAM_DEVICE_BATCH_MB", "192")
    assert be.signature_many(eng, path, ["c"] * 300 + ["nowhere"], regions + [(0, 30, 10, 20, 5, C, 0, 0, 63)]) == host + [[0] * 10]
    monkeypatch.setenv("VAPOR_BAM_DEVICE", "0")
    assert be.signature_many(eng, path, ["c"] * 300, regions) == host


def test_a_damaged_block_sends_its_regions_to_the_host_route_and_no_other(eng, many, tmp_path):
    good, regions, _recs = many
    raw = bytearray(open(good, "rb").read())
    bl = TB._blocks(bytes(raw))
    off, bsize, _xlen = bl[len(bl) // 2]
    raw[off + bsize - 8] ^= 0x40                     # the block's CRC
    bad = str(tmp_path / "bad.bam")
    open(bad, "wb").write(bytes(raw))
    shutil.copy(good + ".bai", bad + ".bai")
    b = bamio.BamFile(bad)
    g = bamio.BamFile(good)
    out, status, chunks = device(eng, b, ["c"] * 300, regions)
    n_bad = 0
    for k, rg in enumerate(regions):
        # a region touches the block iff one of its chunks' file ranges holds the block's offset
        touches = any((cs >> 16) <= off and (off < (ce >> 16) or (off == (ce >> 16) and (ce & 0xFFFF))) for cs, ce in chunks[k])
        assert status[k] == (REG_BLOCK if touches else 0), (k, status[k], touches)
        if touches:
            n_bad += 1
            assert out[k] == [0] * 10
            with pytest.raises(ValueError):          # the host route's answer for such a region: the file is damaged
                b.signature_native(0, rg)
        else:
            assert out[k] == g.signature_native(0, rg) == b.signature_native(0, rg)
    assert 1 <= n_bad < 150, n_bad
    # signature_many hands the region to the host route, which words the error
    be = seqio.InProcessBam()
    with pytest.raises(ValueError, match="vapor_bam_signature"):
        be.signature_many(eng, bad, ["c"] * 300, regions)
    ok = [k for k in range(300) if status[k] == 0]
    assert be.signature_many(eng, bad, ["c"] * len(ok), [regions[k] for k in ok]) == [out[k] for k in ok]
    b.close()
    g.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the CLI from files
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cmd", ["bed", "vcf"])
def test_cli_from_files_equals_the_host_routes_and_the_closed_form(cmd, tmp_path, monkeypatch):
    w = synth.make_signature_world(seed=21, layers=SC.LAYERS, jitter=SC.JITTER)
    expect = SC.closed_form(w, synth.SIGNATURE_SPECS)
    fa, bam = synth.write_world_files(w, str(tmp_path), block_size=8192)
    text = synth.bed_text(w) if cmd == "bed" else synth.vcf_text(w)
    seqio.set_backend(None)
    pipeline.set_engine(None)
    calls = []
    orig = Engine.bam_signature_device
    monkeypatch.setattr(Engine, "bam_signature_device", lambda self, *a, **k: calls.append(len(a[1])) or orig(self, *a, **k))
    try:
        table, _ = SC.run_main(tmp_path, "dev", cmd, text, ["--signatures"], fa, bam)
        n_dev = sum(calls)
        plain, _ = SC.run_main(tmp_path, "plain", cmd, text, (), fa, bam)
        monkeypatch.setenv("VAPOR_BAM_DEVICE", "0")
        seqio.set_backend(None)
        calls.clear()
        host, _ = SC.run_main(tmp_path, "host", cmd, text, ["--signatures"], fa, bam)
        assert not calls
        monkeypatch.delenv("VAPOR_BAM_DEVICE")
        monkeypatch.setenv("VAPOR_BAM_NATIVE", "0")
        seqio.set_backend(None)
        py, _ = SC.run_main(tmp_path, "py", cmd, text, ["--signatures"], fa, bam)
        assert not calls
    finally:
        monkeypatch.delenv("VAPOR_BAM_NATIVE", raising=False)
        seqio.set_backend(None)
        pipeline.set_engine(None)
    assert table == host == py
    rows = [r.split("\t") for r in table.splitlines()]
    assert "\n".join("\t".join(r[:-6]) for r in rows) + "\n" == plain
    by_contig = {(r[0] if cmd == "bed" else r[0].split(":")[0]): r[-6:] for r in rows[1:]}
    n_loci = 0
    for l, e in zip(w.loci, expect):
        if cmd == "vcf" and l.svtype == "TANDUP":
            continue
        n_loci += 1
        assert by_contig[l.chrom] == e, (l, by_contig[l.chrom], e)
    assert len(by_contig) == n_loci and n_dev > n_loci                   # (a locus above P is two regions)

"""Alt and ref alignments on the device (`--support`, DESIGN.md 4.22: vapor_bam_support_device - bgzf_inflate_kernel,
bam_support_kernel) against the native host reader (vapor_bam_support), the Python statement (support.answer over bamio's records)
and the brute force of tests/test_support_cpu.py: per region the seven words and the status, exactly - one region per way the
kernel can go wrong, 300 regions in one call and split over many, a file with a damaged block (a handled status), and the CLI's
tables from files."""
import shutil

import numpy as np
import pytest

import test_bamio as TB
import test_gpu_depth as GD
import test_gpu_signature as GS
import test_signature_cpu as SC
import test_support_cpu as UC
from vapor_amd import _lib as L
from vapor_amd import bamio, pipeline, seqio, support, synth
from vapor_amd.engine import Engine

pytestmark = pytest.mark.gpu

REG_BLOCK = 5
C, T, F, G = UC.C, UC.T, UC.F, UC.G
NCAP = UC.NCAP
M, I, D, N, S, H, PAD, EQ, X = range(9)
LC0, RC0, LC1, RC1, GAP, INSOP, REF0, REF1 = 1, 2, 4, 8, 16, 32, 64, 128
ALL = 255
CR = 15 | REF0 | REF1            # the clip bits and reference support: no operation counts as GAP or INSOP


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def device(eng, b, chroms, regions):
    """engine.bam_support_device over the regions' .bai chunks: (seven words per region, status per region, chunks per region)."""
    tids = [b.tid[c] for c in chroms]
    chunk_first, flat, per = [0], [], []
    for t, rg in zip(tids, regions):
        ch = b.index.chunks(t, int(rg[0]), int(rg[1])) if rg[1] > rg[0] else []
        per.append(ch)
        for c in ch:
            flat += [c[0], c[1]]
        chunk_first.append(len(flat) // 2)
    with b.handle(L.load()) as tl:
        out, status = eng.bam_support_device(tl["native"], tids, np.asarray(regions, dtype=np.int64).reshape(-1, 11), chunk_first,
                                             np.asarray(flat, dtype=np.uint64))
    return [[int(x) for x in o] for o in out], status.tolist(), per


def statement(b, chrom, rg):
    recs = [(r[1], r[2]) for r in b.fetch_raw(chrom, int(rg[0]) + 1, int(rg[1]), exclude_more=support.EXCLUDE)] if rg[1] > rg[0] else []
    return support.answer(recs, rg)


# ------------------------------------------------------------------------------------------------------------------------------
# one region per way the kernel can go wrong
# ------------------------------------------------------------------------------------------------------------------------------
N_OPS = GS.N_OPS                 # 0, 1, 2, 3, 63, 64, 65, 66, 128, 129 and 4 000 operations
ops_of, span_of = GS.ops_of, GS.span_of
BLOCK = 4096
X0, X1 = 20000, 20600            # the breakpoints of contig `rule`
FAR = 39000                      # a second target of contig `rule` that nothing reaches
ALT = [((1, M), (1, EQ))[i % 2] for i in range(4000)]      # operations of one base, one a lane
T4000 = 40000                    # the 4 000-operation record with a D in its first tile and an N in its last


@pytest.fixture(scope="module")
def designed(tmp_path_factory):
    rows = []                                        # (name, tid, pos0, ops, mapq, flag)
    refs = [("ops", 80000), ("edge", 60000), ("cg", 120000), ("rule", 40000), ("two", 140000), ("flt", 50000), ("none", 9000)]
    rows.append(("start", 0, 0, [(300, M)], 60, 0))                                       # x - F < 0 for a target below 51
    for k, n in enumerate(N_OPS):
        rows.append(("n%d" % n, 0, 5000 * k + 1000, ops_of(n), 60, 0))
        rows.append(("m%d" % n, 0, 5000 * k + 1030, [(45, H), (900, M)], 60, 0))          # a neighbour in the same window
    # the trailing clip as operation 63, 64 and 65 (one S of C bases: lane 63 of the first tile, lanes 0 and 1 of the second)
    for k, n in enumerate((64, 65, 66)):
        rows.append(("t%d" % n, 1, 1000 + 2000 * k, ALT[:n - 1] + [(C, S)], 60, 0))
    # a blocking D on lane 63 of the first tile and nothing but M behind it; a blocking I on lane 0 of the second tile
    rows.append(("b63", 1, 10000, ALT[:63] + [(40, D), (400, M)], 60, 0))
    rows.append(("b64", 1, 12000, ALT[:64] + [(40, I), (400, M)], 60, 0))
    # a counted GAP in tile 0 of a record of two tiles that spans both targets: cg wins over ref (no operation reaches gmin)
    rows.append(("cgwin", 1, 20000, [(200, M), (600, D)] + ALT[:100] + [(300, M)], 60, 0))
    # 4 000 operations: a D of 40 in the first tile, an N of 40 in the last, 62 tiles of one-base operations between them
    rows.append(("t4000", 1, T4000, [(100, M), (40, D)] + ALT[:3994] + [(40, N), (200, M), (35, S), (5, H)], 60, 0))
    # CG:B,I: 70 000 operations that reach 60 000 with a GAP of 800 and a trailing clip behind it
    rows.append(("cg", 2, 60000 - 34998, [(1, M) if j % 2 == 0 else (1, I) for j in range(69996)] + [(800, D), (0, M), (33, S), (9, H)], 60, 0))
    rows.append(("cg_after", 2, 95000, [(40, S), (400, M)], 60, 0))
    # the rule at its edges, on contig `rule`, every record around X0
    x = X0
    for name, pos, ops in (
            ("pos_at", x - F, [(400, M)]), ("pos_in", x - F + 1, [(400, M)]), ("q_at", x + F - 400, [(400, M)]), ("q_in", x + F - 401, [(400, M)]),
            ("d_ends_at", x - F - 140, [(100, M), (40, D), (400, M)]), ("d_ends_in", x - F + 1 - 140, [(100, M), (40, D), (400, M)]),
            ("d_starts_in", x - 200, [(200 + F - 1, M), (40, N), (100, M)]), ("d_starts_at", x - 200, [(200 + F, M), (40, N), (100, M)]),
            ("i_before", x - 200, [(200 - F - 1, M), (40, I), (400, M)]), ("i_first", x - 200, [(200 - F, M), (40, I), (400, M)]),
            ("i_last", x - 200, [(200 + F, M), (40, I), (400, M)]), ("i_behind", x - 200, [(200 + F + 1, M), (40, I), (400, M)]),
            ("d_short", x - 200, [(200, M), (G - 1, D), (200, M)]), ("d_long", x - 200, [(200, M), (G, D), (200, M)]),
            ("i_short", x - 200, [(200, M), (G - 1, I), (200, M)]), ("i_long", x - 200, [(200, M), (G, I), (200, M)]),
            ("ins_mid", x - 200, [(500, M), (600, I), (500, M)]), ("clip_and_span", x - 55, [(40, S), (400, M)]),
            ("gap", x - 300, [(300, M), (600, D), (300, M)]), ("lclip1", X1 + 3, [(12, H), (20, S), (300, M)]), ("rclip0", x - 300 + 7, [(300, M), (40, S)]),
            ("lclip0", x + 5, [(40, S), (300, M)]), ("rclip1", X1 - 4 - 300, [(300, M), (40, S)]),
            ("cov_first", x, [(10, M)]), ("cov_behind", x + 1, [(10, M)]), ("cov_before", x - 10, [(10, M)]), ("cov_last", x - 9, [(10, M)]),
            ("all_clip", x, [(100, H), (100, S)]), ("no_cigar", x, [])):
        rows.append((name, 3, pos, ops, 60, 0))
    # two .bai chunks: a long record in a high bin, records of another leaf bin behind it in the file, then the window's own
    rows.append(("long", 4, 10000, [(35000, M), (40, S)], 60, 0))
    for i in range(40):
        rows.append(("gap%d" % i, 4, 12000 + 10 * i, [(300, M)], 60, 0))
    for i in range(12):
        rows.append(("own%d" % i, 4, 39000 + 150 * i, [(35, S), (500, M), (40, D), (500, EQ), (35, S)], 60, 0))
    rows.append(("at_w3", 4, 40051, [(40, S), (700, M)], 60, 0))
    # filtered records first, three in a row, last; and a stretch where every record is filtered
    for i, flag in enumerate((0x4, 0, 0, 0x100, 0x200, 0x400, 0, 0x800, 0, 0x400)):
        rows.append(("f%d" % i, 5, 2000 + 3 * i, [(40, S), (1000, M)], 60, flag))
    for i in range(5):
        rows.append(("all%d" % i, 5, 30000 + 5 * i, [(600, M)], 60, (0x100, 0x400, 0x4, 0x200, 0x704)[i]))
    rows.sort(key=lambda r: (r[1], r[2]))
    path = str(tmp_path_factory.mktemp("gpu_support") / "designed.bam")
    SC.write_rows(path, refs, rows, block_size=BLOCK)
    # a record header across two BGZF blocks, by design: the file again with a block size that puts a block boundary 18 bytes
    # behind the start of the 4000-operation record (where a record starts in the inflated stream does not depend on the blocks)
    q = [q for q, name in GD._record_starts(path) if name == "t4000"][0]
    k = max(1, round(q / BLOCK))
    block = (q + 18) // k
    SC.write_rows(path, refs, rows, block_size=block)
    by_chrom = {name: [(r[2], r[3], r[4], r[5]) for r in rows if r[1] == t] for t, (name, _n) in enumerate(refs)}
    return path, by_chrom, block


def around(x0, x1, tol=T, mc=C, nmin=0, nmax=NCAP, mask=ALL, flank=F, gmin=G):
    reach = max(tol, flank)
    return (max(min(x0, x1) - reach - 1, 0), max(x0, x1) + reach + 1, x0, x1, tol, mc, nmin, nmax, mask, flank, gmin)


def _cases():
    out = []
    for k, n in enumerate(N_OPS):
        pos = 5000 * k + 1000
        end = pos + span_of(ops_of(n))
        mid = (pos + end) // 2
        out.append(("%d operations, its ends" % n, "ops", around(pos, end, mask=15 | REF0 | REF1)))
        out.append(("%d operations, every bit" % n, "ops", around(pos, end, nmin=1, nmax=10)))
        out.append(("%d operations, its middle" % n, "ops", around(mid, mid, tol=5, flank=8, gmin=6, nmin=1, nmax=10, mask=REF0 | REF1)))
        out.append(("%d operations, its middle, blocked" % n, "ops", around(mid, mid, tol=5, flank=8, gmin=2, nmin=1, nmax=10, mask=REF0 | REF1)))
    for k, n in enumerate((64, 65, 66)):
        pos = 1000 + 2000 * k
        out.append(("the trailing clip as operation %d" % (n - 1), "edge", around(pos, pos + n - 1, mask=RC1 | REF1)))
    end4000 = T4000 + 140 + 3994
    out += [
        ("a blocking D on lane 63", "edge", around(10060, 10060, mask=CR)),
        ("the D on lane 63 below gmin", "edge", around(10060, 10060, mask=CR, gmin=41)),
        ("a blocking I on lane 0 of the second tile", "edge", around(12064, 12064, mask=CR)),
        ("the I on lane 0 below gmin", "edge", around(12064, 12064, mask=CR, gmin=41)),
        ("a counted GAP in tile 0 of a spanner of both targets", "edge", around(20200, 20800, nmin=300, nmax=1200, gmin=601)),
        ("the same without the GAP bit", "edge", around(20200, 20800, nmin=300, nmax=1200, gmin=601, mask=ALL & ~GAP)),
        ("the same, the GAP blocks", "edge", around(20200, 20800, nmin=300, nmax=1200, mask=ALL & ~GAP)),
        ("blocked in the first and in the last tile of 4 000 operations", "edge", around(T4000 + 100, end4000 + 10, mask=REF0 | REF1)),
        ("4 000 operations, nothing reaches gmin", "edge", around(T4000 + 100, end4000 + 10, mask=REF0 | REF1, gmin=41)),
        ("4 000 operations, the first tile blocks alone", "edge", around(T4000 + 100, end4000 + 100, mask=REF0 | REF1)),
        ("4 000 operations, the last tile blocks alone", "edge", around(T4000 + 1000, end4000 + 10, mask=REF0 | REF1)),
        ("4 000 operations, its trailing clip", "edge", around(T4000, end4000 + 240, mask=RC1 | REF1)),
        ("CG:B,I of 70 000 operations", "cg", around(60000, 60800, nmin=400, nmax=1600)),
        ("CG:B,I, its clip without the GAP bit", "cg", around(60000, 60800, nmin=400, nmax=1600, mask=ALL & ~GAP)),
        ("CG:B,I, its I operations", "cg", around(59990, 60000, tol=5, nmin=1, nmax=1, mask=INSOP | REF0 | REF1, gmin=2)),
        ("CG:B,I, every I blocks", "cg", around(59000, 59000, mask=CR, gmin=1)),
        ("the rule's edges", "rule", around(X0, FAR, mask=CR)),
        ("g + 1", "rule", around(X0, FAR, mask=CR, gmin=G + 1)),
        ("g above every operation", "rule", around(X0, FAR, mask=CR, gmin=1 << 40)),
        ("F + 1", "rule", around(X0, FAR, mask=CR, flank=F + 1)),
        ("F - 1", "rule", around(X0, FAR, mask=CR, flank=F - 1)),
        ("F 1", "rule", around(X0, FAR, mask=CR, flank=1)),
        ("F 65535", "rule", around(X0, FAR, mask=CR, flank=65535)),
        ("tol above F", "rule", around(X0, FAR, mask=CR, tol=60)),
        ("tol 0", "rule", around(X0, FAR, mask=CR, tol=0)),
        ("tol 255", "rule", around(X0, FAR, mask=CR, tol=255, flank=300)),
        ("x0 == x1", "rule", around(X0, X0, mask=CR)),
        ("both targets, a TANDUP's mask", "rule", around(X0, X1, nmin=300, nmax=1200, mask=LC0 | RC1 | INSOP | REF0 | REF1)),
        ("both targets, a DEL's mask", "rule", around(X0, X1, nmin=300, nmax=1200, mask=RC0 | LC1 | GAP | REF0 | REF1)),
        ("both targets, every bit", "rule", around(X0, X1, nmin=300, nmax=1200)),
        ("bits 6 and 7 off", "rule", around(X0, X1, nmin=300, nmax=1200, mask=63)),
        ("all bits off", "rule", around(X0, X1, nmin=300, nmax=1200, mask=0)),
        ("min_clip C + 11", "rule", around(X0, X1, mask=CR, mc=C + 11)),
    ]
    out += [("bit %d alone" % bit, "rule", around(X0, X1, nmin=300, nmax=1200, mask=1 << bit)) for bit in range(8)]
    out += [
        ("two .bai chunks; a spanner in a high bin, a record at w3", "two", around(40000, 40000)),
        ("filtered first, three in a row, last", "flt", around(2500, 2500)),
        ("all filtered", "flt", around(30300, 30300)),
        ("a contig without records", "none", around(1000, 2000)),
        ("an empty window", "two", (40000, 40000, 39990, 39990, T, C, 0, 0, ALL, F, G)),
        ("x - F < 0", "ops", (0, 200, 30, 100, T, C, 0, 0, ALL, F, G)),
        ("x - F = 0", "ops", (0, 200, F, F, T, C, 0, 0, ALL, F, G)),
    ]
    return out


def test_every_designed_region_equals_host_statement_and_model(eng, designed):
    path, by_chrom, block = designed
    b = bamio.BamFile(path)
    cases = _cases()
    assert len({c[0] for c in cases}) == len(cases)
    chroms, regions = [c[1] for c in cases], [c[2] for c in cases]
    out, status, chunks = device(eng, b, chroms, regions)
    assert status == [0] * len(cases), status
    for (name, chrom, rg), got in zip(cases, out):
        host = b.support_native(b.tid[chrom], rg)
        want = UC.brute(by_chrom[chrom], rg)
        assert got == host == want == statement(b, chrom, rg), (name, got, host, want)
    by_name = {c[0]: (g, ch) for c, g, ch in zip(cases, out, chunks)}
    # the properties the cases are there for
    for n in N_OPS:
        ends, mid, blocked = (by_name["%d operations, %s" % (n, w)][0] for w in ("its ends", "its middle", "its middle, blocked"))
        # the record's own clips (the neighbour adds a leading one): none without CIGAR, none for a single M, a leading one from 2 on,
        # a trailing one from 3 on - as 20S + 15H, in two tiles at 65 and 129 (without operations both targets are the record's
        # start, where the neighbour's clip counts twice)
        assert ends[0] == 0 and ends[1] == (2 if n >= 2 else 1) and ends[2] == (1 if n >= 3 or n == 0 else 0), (n, ends)
        # with the CIGAR bits the pattern's operations count: the record is cg, and its clips are not counted again
        every = by_name["%d operations, every bit" % n][0]
        assert every[:3] == ([1, 1, 0] if n >= 63 else ends[:3]), (n, every)
        # the record holds its middle when it has operations - 200 M up to three, the pattern beyond, whose D of 2 and N of 5 every
        # 16 bases block at gmin 2 and not at 6; the neighbour, 900 M from 30 bases behind its start, holds it up to 1 800 bases
        near = 1 if 30 + 8 <= span_of(ops_of(n)) // 2 <= 930 - 8 else 0
        assert mid[3:5] == [(n >= 1) + near] * 2 and blocked[3:5] == [(1 <= n <= 3) + near] * 2, (n, mid, blocked)
    assert all(by_name["the trailing clip as operation %d" % k][0] == [0, 0, 1, 0, 0, 1, 0] for k in (63, 64, 65))
    assert by_name["a blocking D on lane 63"][0] == [0, 0, 0, 0, 0, 1, 1] and by_name["the D on lane 63 below gmin"][0] == [0, 0, 0, 1, 1, 1, 1]
    assert by_name["a blocking I on lane 0 of the second tile"][0] == [0, 0, 0, 0, 0, 1, 1] and by_name["the I on lane 0 below gmin"][0] == [0, 0, 0, 1, 1, 1, 1]
    assert by_name["a counted GAP in tile 0 of a spanner of both targets"][0] == [1, 0, 0, 0, 0, 1, 1]
    assert by_name["the same without the GAP bit"][0] == [0, 0, 0, 1, 1, 1, 1] and by_name["the same, the GAP blocks"][0] == [0, 0, 0, 0, 0, 1, 1]
    assert by_name["blocked in the first and in the last tile of 4 000 operations"][0] == [0, 0, 0, 0, 0, 1, 1]
    assert by_name["4 000 operations, nothing reaches gmin"][0] == [0, 0, 0, 1, 1, 1, 1]
    assert by_name["4 000 operations, the first tile blocks alone"][0] == [0, 0, 0, 0, 1, 1, 1]
    assert by_name["4 000 operations, the last tile blocks alone"][0] == [0, 0, 0, 1, 0, 1, 1]
    assert by_name["4 000 operations, its trailing clip"][0] == [0, 0, 1, 0, 0, 1, 0]
    assert by_name["CG:B,I of 70 000 operations"][0] == [1, 0, 0, 0, 0, 1, 0] and by_name["CG:B,I, its clip without the GAP bit"][0] == [0, 0, 1, 0, 0, 1, 0]
    assert by_name["CG:B,I, its I operations"][0] == [1, 0, 0, 0, 0, 1, 1] and by_name["CG:B,I, every I blocks"][0] == [0, 0, 0, 0, 0, 1, 1]
    edges = by_name["the rule's edges"][0]
    # the spanners of X0: pos_at, q_at, d_ends_at, d_starts_at, i_before, i_behind, d_short, i_short, ins_mid (its I is 300 bases
    # off), clip_and_span (its clip is 55 bases off); rclip0 ends 7 bases behind X0 and lclip0 starts 5 behind it: two clips
    assert edges[:5] == [0, 2, 0, 10, 0], edges
    # d_long and i_long pass at g = 31; at 2^40 the four at the flank's edges and the gap as well
    assert by_name["g + 1"][0][3] == 10 + 2 and by_name["g above every operation"][0][3] == 10 + 2 + 4 + 1
    # F + 1: the six records that reach or stay clear by exactly one base fall out; F - 1: the six one base short come in
    assert by_name["F + 1"][0][3] == 10 - 6 and by_name["F - 1"][0][3] == 10 + 6
    assert by_name["F 65535"][0][3] == 0 and by_name["F 1"][0][3] > 14
    assert by_name["tol above F"][0][1:4] == [3, 0, 9] and by_name["tol 0"][0][1] == 0 and by_name["x0 == x1"][0][3:5] == [10, 10]
    assert by_name["both targets, a TANDUP's mask"][0][0] == 1 and by_name["both targets, a TANDUP's mask"][0][3] == 9
    assert by_name["both targets, a DEL's mask"][0][:3] == [1, 1, 1] and by_name["both targets, a DEL's mask"][0][3] == 10
    every = by_name["both targets, every bit"][0]
    assert every[0] == 2 and by_name["bits 6 and 7 off"][0] == every[:3] + [0, 0] + every[5:] and by_name["all bits off"][0] == [0] * 5 + every[5:]
    assert by_name["min_clip C + 11"][0][1:3] == [0, 0]
    for bit in range(8):
        got = by_name["bit %d alone" % bit][0]
        assert got[5:] == every[5:] and sum(got[:5]) > 0 and [k for k in range(5) if got[k]] == [[1], [1], [2], [2], [0], [0], [3], [4]][bit], (bit, got)
    two = by_name["two .bai chunks; a spanner in a high bin, a record at w3"]
    assert len(two[1]) == 2 and two[0][3] == two[0][4] >= 2 and two[0][5] >= 3
    assert by_name["filtered first, three in a row, last"][0] == [0, 0, 0, 5, 5, 5, 5] and by_name["all filtered"][0] == [0] * 7
    assert by_name["a contig without records"][0] == [0] * 7 and by_name["an empty window"][0] == [0] * 7 and by_name["an empty window"][1] == []
    assert by_name["x - F < 0"][0] == [0, 0, 0, 0, 1, 1, 1] and by_name["x - F = 0"][0] == [0, 0, 0, 1, 1, 1, 1]
    # a record header across two BGZF blocks is among the records walked: the 4000-operation record's
    starts = dict((name, q) for q, name in GD._record_starts(path))
    assert starts["t4000"] // block + 1 == (starts["t4000"] + 35) // block
    b.close()


def test_with_the_handles_filter(eng, designed):
    path, by_chrom, _block = designed
    b = bamio.BamFile(path)
    rg = around(2500, 2500)
    seen = []
    for flt in ((0, 0), (0, 0x800), (61, 0), (60, 0x800)):
        b.set_filter(*flt)
        out, status, _ = device(eng, b, ["flt", "rule"], [rg, around(X0, X1, nmin=300, nmax=1200)])
        assert status == [0, 0]
        assert out[0] == b.support_native(b.tid["flt"], rg) == UC.brute(by_chrom["flt"], rg, *flt) == statement(b, "flt", rg)
        assert out[1] == UC.brute(by_chrom["rule"], around(X0, X1, nmin=300, nmax=1200), *flt)
        seen.append(out[0][3])
    assert seen == [5, 4, 0, 4]
    b.set_filter(0, 0)
    b.set_dedup(True)
    assert device(eng, b, ["flt"], [rg])[0][0][3] == 5                   # --dedup-qname has no effect
    b.close()


def test_refused_regions_and_arguments(eng, designed):
    path, _, _block = designed
    b = bamio.BamFile(path)
    with b.handle(L.load()) as tl:
        ch = np.asarray(b.index.chunks(0, 0, 5000), dtype=np.uint64).reshape(-1)
        good = (0, 400, 100, 100, T, C, 0, 10, ALL, F, G)
        bad = [good[:k] + (v,) + good[k + 1:] for k, v in ((0, 401), (1, 1 << 31), (4, -1), (4, 256), (6, 11), (0, -1), (9, 0), (9, 65536), (10, 0))]
        regions = np.asarray([good] + bad + [good], dtype=np.int64)
        n = len(regions)
        first = np.arange(n + 1, dtype=np.int32) * (len(ch) // 2)
        out, status = eng.bam_support_device(tl["native"], [0] * (n - 1) + [-1], regions, first, np.tile(ch, n))
        assert status.tolist() == [0] + [2] * (n - 1) and out[1:].tolist() == [[0] * 7] * (n - 1) and out[0].tolist() == b.support_native(0, good)
        assert out[0].tolist() == [0, 0, 0, 1, 1, 1, 1]
        out, status = eng.bam_support_device(tl["native"], [], np.zeros((0, 11), dtype=np.int64), [0], [])
        assert len(out) == 0 and len(status) == 0
    b.close()


# ------------------------------------------------------------------------------------------------------------------------------
# many regions
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many(tmp_path_factory):
    rng = np.random.default_rng(13)
    n = 60000
    rows = [("m%d" % i, 0) + r for i, r in enumerate(SC.seeded_records(rng, 2500, 0, n - 3000, clip_p=0.8))]
    path = str(tmp_path_factory.mktemp("gpu_support_many") / "many.bam")
    SC.write_rows(path, [("c", n)], rows, block_size=20000)
    regions = []
    for _ in range(300):
        x0 = int(rng.integers(300, n - 3000))
        x1 = x0 + int(rng.integers(0, 130))
        tol = int(rng.choice([0, 5, T, 120, 255]))
        flank = int(rng.choice([1, 5, F, 120, 300]))
        nmin = int(rng.integers(0, 60))
        regions.append(around(x0, x1, tol=tol, mc=int(rng.integers(1, 45)), nmin=nmin, nmax=nmin + int(rng.integers(0, 120)), mask=int(rng.integers(0, 256)),
                              flank=flank, gmin=int(rng.choice([1, 10, G, 1000]))))
    return path, regions, [r[2:] for r in rows]


def test_300_regions_in_one_call_and_split_and_halved(eng, many, monkeypatch):
    path, regions, recs = many
    b = bamio.BamFile(path)
    out, status, chunks = device(eng, b, ["c"] * 300, regions)
    assert status == [0] * 300
    host = [b.support_native(0, rg) for rg in regions]
    assert out == host
    for g in range(0, 300, 10):
        assert out[g] == statement(b, "c", regions[g]) == UC.brute(recs, regions[g])
    assert all(sum(o[k] > 0 for o in out) > 20 for k in range(7))
    b.close()
    # the same through support_many, its groups so small that the call is split, and a library that refuses more than 8 regions
    # "in one call" so that the groups are halved
    calls = []

    class Refusing:
        def bam_support_device(self, native, tids, *a):
            calls.append(len(tids))
            if len(tids) > 8:
                raise L.VaporHipError(-4, "vapor_bam_support_device: more than 1.5 GB of blocks in one call (use smaller batches)")
            return eng.bam_support_device(native, tids, *a)
    monkeypatch.setenv("VAPOR_BAM_DEVICE_BATCH_MB", "8")
    be = seqio.InProcessBam()
    assert be.support_many(Refusing(), path, ["c"] * 300, regions) == host
    big, small = [c for c in calls if c > 8], [c for c in calls if c <= 8]
    assert len(big) >= 3 and sum(small) == 300 and max(calls) < 300
    calls.clear()
    monkeypatch.setenv("VAPOR_BAM_DEVICE_BATCH_MB", "192")
    assert be.support_many(eng, path, ["c"] * 300 + ["nowhere"], regions + [(0, 30, 10, 20, 5, C, 0, 0, ALL, F, G)]) == host + [[0] * 7]
    monkeypatch.setenv("VAPOR_BAM_DEVICE", "0")
    assert be.support_many(eng, path, ["c"] * 300, regions) == host


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
            assert out[k] == [0] * 7
            with pytest.raises(ValueError):          # the host route's answer for such a region: the file is damaged
                b.support_native(0, rg)
        else:
            assert out[k] == g.support_native(0, rg) == b.support_native(0, rg)
    assert 1 <= n_bad < 150, n_bad
    # support_many hands the region to the host route, which words the error
    be = seqio.InProcessBam()
    with pytest.raises(ValueError, match="vapor_bam_support"):
        be.support_many(eng, bad, ["c"] * 300, regions)
    ok = [k for k in range(300) if status[k] == 0]
    assert be.support_many(eng, bad, ["c"] * len(ok), [regions[k] for k in ok]) == [out[k] for k in ok]
    b.close()
    g.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the CLI from files
# ------------------------------------------------------------------------------------------------------------------------------
SPECS = synth.SUPPORT_SPECS              # every type short and long, het, hom and ref: 24 loci


@pytest.mark.parametrize("cmd", ["bed", "vcf"])
def test_cli_from_files_equals_the_host_routes_and_the_closed_form(cmd, tmp_path, monkeypatch):
    w = synth.make_support_world(seed=21, specs=SPECS, layers=UC.LAYERS)
    expect = UC.closed_form(SPECS)
    fa, bam = synth.write_world_files(w, str(tmp_path), block_size=8192)
    text = synth.bed_text(w) if cmd == "bed" else synth.vcf_text(w)
    seqio.set_backend(None)
    pipeline.set_engine(None)
    calls = []
    orig = Engine.bam_support_device
    monkeypatch.setattr(Engine, "bam_support_device", lambda self, *a, **k: calls.append(len(a[1])) or orig(self, *a, **k))
    try:
        table, _ = SC.run_main(tmp_path, "dev", cmd, text, ["--support"], fa, bam)
        n_dev = sum(calls)
        calls.clear()
        # a plain run takes nothing of the new path: no support call, and its table is the option's without the nine columns
        plain, _ = SC.run_main(tmp_path, "plain", cmd, text, (), fa, bam)
        assert not calls and "VaPoR_SUP" not in plain
        monkeypatch.setenv("VAPOR_BAM_DEVICE", "0")
        seqio.set_backend(None)
        host, _ = SC.run_main(tmp_path, "host", cmd, text, ["--support"], fa, bam)
        assert not calls
        monkeypatch.delenv("VAPOR_BAM_DEVICE")
        monkeypatch.setenv("VAPOR_BAM_NATIVE", "0")
        seqio.set_backend(None)
        py, _ = SC.run_main(tmp_path, "py", cmd, text, ["--support"], fa, bam)
        assert not calls
    finally:
        monkeypatch.delenv("VAPOR_BAM_NATIVE", raising=False)
        seqio.set_backend(None)
        pipeline.set_engine(None)
    assert table == host == py
    rows = [r.split("\t") for r in table.splitlines()]
    assert rows[0][-9:] == list(support.COLUMNS)
    assert "\n".join("\t".join(r[:-9]) for r in rows) + "\n" == plain
    by_contig = {(r[0] if cmd == "bed" else r[0].split(":")[0]): r[-9:] for r in rows[1:]}
    n_loci = 0
    for l, e in zip(w.loci, expect):
        if cmd == "vcf" and l.svtype == "TANDUP":
            continue
        n_loci += 1
        assert by_contig[l.chrom] == e, (l, by_contig[l.chrom], e)
    assert len(by_contig) == n_loci and n_dev > n_loci                   # (a locus above P is two regions)

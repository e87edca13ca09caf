"""Read depth on the device (`--depth`, DESIGN.md 4.19: vapor_bam_depth_device - bgzf_inflate_kernel, bam_depth_kernel) against
the native host reader (vapor_bam_depth), the Python statement (depth.cover over bamio's records) and a per-base pile-up stated in
tests/test_depth_cpu.py: per region the three sums and the status, exactly - one region per way the kernel can go wrong, 300
regions in one call and split over many, a file with a damaged block (a handled status), and the CLI's tables from files."""
import os
import shutil
import struct
import zlib

import numpy as np
import pytest

import test_bamio as TB
import test_depth_cpu as DC
from vapor_amd import _lib as L
from vapor_amd import bamio, cli, depth, pipeline, seqio, synth
from vapor_amd.engine import Engine

pytestmark = pytest.mark.gpu

REG_BLOCK = 5
TOP = (1 << 31) - 1
MMAX = (1 << 28) - 1            # the longest operation a BAM record holds


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def device(eng, b, chroms, bounds):
    """engine.bam_depth_device over the regions' .bai chunks: (cov per region, status per region, chunks per region)."""
    tids = [b.tid[c] for c in chroms]
    chunk_first, flat, per = [0], [], []
    for t, bd in zip(tids, bounds):
        ch = b.index.chunks(t, int(bd[0]), int(bd[3]))
        per.append(ch)
        for c in ch:
            flat += [c[0], c[1]]
        chunk_first.append(len(flat) // 2)
    with b.handle(L.load()) as tl:
        cov, status = eng.bam_depth_device(tl["native"], tids, np.asarray(bounds, dtype=np.int64).reshape(-1, 4), chunk_first, np.asarray(flat, dtype=np.uint64))
    return [[int(x) for x in c] for c in cov], status.tolist(), per


def statement(b, chrom, bd):
    recs = [(r[1], r[2]) for r in b.fetch_raw(chrom, int(bd[0]) + 1, int(bd[3]), exclude_more=depth.EXCLUDE)] if bd[3] > bd[0] else []
    return depth.cover(recs, bd)


# ------------------------------------------------------------------------------------------------------------------------------
# one region per way the kernel can go wrong
# ------------------------------------------------------------------------------------------------------------------------------
PATTERN = [(3, 0), (2, 2), (1, 1), (4, 8), (5, 3), (2, 7), (6, 4)]        # M D I X N = S: the cursor moves by 16 every seven operations
N_OPS = (0, 1, 63, 64, 65, 129, 4000)
BLOCK = 4096


def _ops(n):
    return [PATTERN[i % len(PATTERN)] for i in range(n)]


def _span(ops):
    return sum(n for n, c in ops if c in DC.ADVANCES)


@pytest.fixture(scope="module")
def designed(tmp_path_factory):
    rows = []                                        # (name, tid, pos0, ops, mapq, flag)
    refs = [("ops", 60000), ("cg", 120000), ("two", 140000), ("flt", 50000), ("none", 9000), ("big", TOP)]
    for k, n in enumerate(N_OPS):
        rows.append(("n%d" % n, 0, 5000 * k + 100, _ops(n), 60, 0))
        rows.append(("m%d" % n, 0, 5000 * k + 130, [(900, 0)], 60, 0))           # a neighbour over the same intervals
    rows.append(("cg", 1, 20000, [(1, 0) if j % 2 == 0 else (1, 2) for j in range(70000)], 60, 0))
    rows.append(("cg_after", 1, 95000, [(400, 0)], 60, 0))
    # two .bai chunks: a long record in a high bin, records of another leaf bin behind it in the file, then the window's own
    rows.append(("long", 2, 10000, [(35000, 0)], 60, 0))
    for i in range(40):
        rows.append(("gap%d" % i, 2, 12000 + 10 * i, [(300, 0)], 60, 0))
    for i in range(12):
        rows.append(("own%d" % i, 2, 39000 + 150 * i, [(500, 0), (40, 2), (500, 7)], 60, 0))
    rows.append(("at_b3", 2, 41000, [(700, 0)], 60, 0))
    rows.append(("behind_b3", 2, 41500, [(700, 0)], 60, 0))
    # filtered records first, three in a row, last; and a stretch where every record is filtered
    for i, flag in enumerate((0x4, 0, 0, 0x100, 0x200, 0x400, 0, 0x800, 0, 0x400)):
        rows.append(("f%d" % i, 3, 2000 + 100 * i, [(1000, 0)], 60, flag))
    for i in range(5):
        rows.append(("all%d" % i, 3, 30000 + 50 * i, [(600, 0)], 60, (0x100, 0x400, 0x4, 0x200, 0x704)[i]))
    # sums above 2^32 from a small file: six records of the longest operations a record holds, to the end of a contig of 2^31 - 1 bases
    for i in range(6):
        rows.append(("big%d" % i, 5, 1000 * i, [(MMAX, 0)] * 7 + [(9, 2), (MMAX - 6000, 8)], 60, 0))
    recs = []
    for name, tid, pos0, ops, mapq, flag in rows:
        # (the bases are not looked at: a record of the longest operations carries none)
        n = DC._seq_len(ops) if tid != 5 else 0
        recs.append((name, tid, pos0, DC._cigar(ops), "ACGT" * (n // 4) + "ACGT"[:n % 4], None, mapq, flag))
    path = str(tmp_path_factory.mktemp("gpu_depth") / "designed.bam")
    bamio.write_bam(path, refs, recs, block_size=BLOCK)
    # a record header across two BGZF blocks, by design: the file again with a block size that puts a block boundary 18 bytes
    # behind the start of the 4000-operation record (where a record starts in the inflated stream does not depend on the blocks)
    q = [q for q, name in _record_starts(path) if name == "n4000"][0]
    k = max(1, round(q / BLOCK))
    assert k < 18
    block = (q + 18) // k
    bamio.write_bam(path, refs, recs, block_size=block)
    by_chrom = {name: [(r[2], r[3], r[4], r[5]) for r in rows if r[1] == t] for t, (name, _n) in enumerate(refs)}
    return path, by_chrom, block


def _record_starts(path):
    """(offset in the inflated stream, QNAME) of every record of a file."""
    raw = open(path, "rb").read()
    datas = [(o, zlib.decompress(raw[o + 12 + x:o + bz - 8], -15)) for o, bz, x in TB._blocks(raw)]
    whole = b"".join(d for _o, d in datas)
    first = bamio.BamFile(path).first_record
    q = sum(len(d) for o, d in datas if o < first >> 16) + (first & 0xFFFF)
    out = []
    while q + 4 <= len(whole):
        l_name = whole[q + 12]
        out.append((q, whole[q + 36:q + 36 + l_name - 1].decode()))
        q += 4 + struct.unpack_from("<i", whole, q)[0]
    return out


def _cases():
    out = []
    for k, n in enumerate(N_OPS):
        pos, span = 5000 * k + 100, _span(_ops(n))
        out.append(("%d operations" % n, "ops", (pos - 50, pos + span // 3, pos + 2 * span // 3 + 1, pos + max(span, 930) + 50)))
    out += [
        ("CG:B,I of 70 000 operations", "cg", (19000, 30001, 80003, 96000)),
        ("CG:B,I, the region ends inside the record", "cg", (19990, 20001, 20101, 20202)),
        ("CG:B,I, the region begins near its end", "cg", (89000, 89991, 90000, 90011)),
        ("two .bai chunks; before b0, behind b3, at b3", "two", (40000, 40300, 40700, 41000)),
        ("one operation over all three intervals", "two", (15000, 20000, 30000, 38000)),
        ("D inside an interval", "two", (39400, 39500, 39545, 39600)),
        ("N and D inside an interval", "ops", (10100, 10110, 10130, 10160)),
        ("filtered first, three in a row, last", "flt", (1500, 2500, 3200, 4500)),
        ("all filtered", "flt", (29000, 30000, 30500, 31000)),
        ("a contig without records", "none", (100, 1100, 2100, 3100)),
        ("empty flanks", "two", (40000, 40000, 41000, 41000)),
        ("empty inside", "two", (39000, 40000, 40000, 41000)),
        ("all three empty", "two", (40000, 40000, 40000, 40000)),
        ("b0 = 0", "ops", (0, 0, 150, 200)),
        ("sums above 2^32", "big", (0, 1 << 30, TOP - 1, TOP)),
        ("sums above 2^32, from 2^30 on", "big", (1 << 30, (1 << 30) + 5, TOP, TOP)),
        ("the whole contig inside", "big", (0, 0, TOP, TOP)),
    ]
    return out


def _closed_form_big(bd):
    """The records of contig `big` are two runs each: [p, p + 7 MMAX) and [p + 7 MMAX + 9, p + 8 MMAX + 9 - 6000), p = 1000 i."""
    cov = [0, 0, 0]
    for i in range(6):
        p = 1000 * i
        for lo, hi in ((p, p + 7 * MMAX), (p + 7 * MMAX + 9, p + 8 * MMAX + 9 - 6000)):
            for k in range(3):
                cov[k] += max(0, min(hi, bd[k + 1]) - max(lo, bd[k]))
    return cov


def test_every_designed_region_equals_host_statement_and_model(eng, designed):
    path, by_chrom, block = designed
    b = bamio.BamFile(path)
    cases = _cases()
    chroms, bounds = [c[1] for c in cases], [c[2] for c in cases]
    cov, status, chunks = device(eng, b, chroms, bounds)
    assert status == [0] * len(cases), status
    for (name, chrom, bd), got in zip(cases, cov):
        host = b.depth_native(b.tid[chrom], bd)
        want = _closed_form_big(bd) if chrom == "big" else DC.pile(by_chrom[chrom], bd)
        assert got == host == want == statement(b, chrom, bd), (name, got, host, want)
    by_name = {c[0]: (g, ch) for c, g, ch in zip(cases, cov, chunks)}
    # the properties the cases are there for
    assert len(by_name["two .bai chunks; before b0, behind b3, at b3"][1]) == 2
    assert by_name["sums above 2^32"][0][1] > 1 << 32 and sum(by_name["the whole contig inside"][0]) > 1 << 33
    assert by_name["a contig without records"][0] == [0, 0, 0] and by_name["all filtered"][0] == [0, 0, 0]
    assert by_name["all three empty"][0] == [0, 0, 0] and by_name["empty inside"][0][1] == 0 and by_name["empty flanks"][0][0::2] == [0, 0]
    assert all(x > 0 for x in by_name["4000 operations"][0]) and all(x > 0 for x in by_name["CG:B,I of 70 000 operations"][0])
    # the record at pos == b3 covers nothing of its region, and everything of a region that holds it
    assert device(eng, b, ["two"], [(41000, 41000, 41700, 41700)])[0][0][1] == DC.pile(by_chrom["two"], (41000, 41000, 41700, 41700))[1] >= 700
    # a record header across two BGZF blocks is among the records walked: the 4000-operation record's
    starts = dict((name, q) for q, name in _record_starts(path))
    assert starts["n4000"] // block + 1 == (starts["n4000"] + 35) // block
    b.close()


def test_with_the_handles_filter(eng, designed):
    path, by_chrom, block = designed
    b = bamio.BamFile(path)
    bd = (1500, 2500, 3200, 4500)
    seen = []
    for flt in ((0, 0), (0, 0x800), (61, 0), (60, 0x800)):
        b.set_filter(*flt)
        cov, status, _ = device(eng, b, ["flt", "two"], [bd, (40000, 40300, 40700, 41000)])
        assert status == [0, 0]
        assert cov[0] == b.depth_native(b.tid["flt"], bd) == DC.pile(by_chrom["flt"], bd, *flt) == statement(b, "flt", bd)
        seen.append(cov[0])
    assert seen[0] != seen[1] and seen[2] == [0, 0, 0] and seen[3] == seen[1]
    b.set_filter(0, 0)
    b.set_dedup(True)
    assert device(eng, b, ["flt"], [bd])[0][0] == seen[0]                   # --dedup-qname has no effect on depth
    b.close()


def test_refused_regions_and_arguments(eng, designed):
    path, _, _block = designed
    b = bamio.BamFile(path)
    with b.handle(L.load()) as tl:
        ch = np.asarray(b.index.chunks(0, 0, 5000), dtype=np.uint64).reshape(-1)
        bounds = np.asarray([(0, 100, 200, 300), (5, 4, 6, 9), (0, 5, 9, 1 << 31), (-1, 5, 9, 12), (0, 100, 200, 300)], dtype=np.int64)
        first = np.arange(6, dtype=np.int32) * (len(ch) // 2)
        cov, status = eng.bam_depth_device(tl["native"], [0, 0, 0, 0, -1], bounds, first, np.tile(ch, 5))
        assert status.tolist() == [0, 2, 2, 2, 2] and cov[1:].tolist() == [[0, 0, 0]] * 4 and cov[0].tolist() == b.depth_native(0, bounds[0])
        cov, status = eng.bam_depth_device(tl["native"], [], np.zeros((0, 4), dtype=np.int64), [0], [])
        assert len(cov) == 0 and len(status) == 0
    b.close()


# ------------------------------------------------------------------------------------------------------------------------------
# many regions
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many(tmp_path_factory):
    rng = np.random.default_rng(12)
    n = 400000
    contig = synth.random_dna(rng, 8000)
    recs = []
    for i in range(420):
        pos = int(rng.integers(0, n - 9000))
        read, cg = synth.mutate(rng, contig[:int(rng.integers(300, 7000))])
        recs.append(("m%d" % i, 0, pos, cg, read, None, int(rng.integers(0, 61)), int(rng.choice([0, 0, 0, 16, 0x800, 0x400]))))
    path = str(tmp_path_factory.mktemp("gpu_depth_many") / "many.bam")
    bamio.write_bam(path, [("c", n)], recs, block_size=20000)
    bounds = []
    for _ in range(300):
        b0 = int(rng.integers(0, n - 50000))
        cuts = np.sort(rng.integers(0, 45000, size=3))
        bounds.append((b0, b0 + int(cuts[0]), b0 + int(cuts[1]), b0 + int(cuts[2])))
    return path, bounds


def test_300_regions_in_one_call_and_split_and_halved(eng, many, monkeypatch):
    path, bounds = many
    b = bamio.BamFile(path)
    cov, status, chunks = device(eng, b, ["c"] * 300, bounds)
    assert status == [0] * 300
    assert sum(len(c) >= 2 for c in chunks) >= 100, sum(len(c) >= 2 for c in chunks)          # several chunks per region
    host = [b.depth_native(0, bd) for bd in bounds]
    assert cov == host
    for g in range(0, 300, 15):
        assert cov[g] == statement(b, "c", bounds[g])
    assert sum(x > 0 for c in cov for x in c) > 600
    b.close()
    # the same through depth_many, its groups so small that the call is split, and a library that refuses more than 8 regions
    # "in one call" so that the groups are halved
    calls = []

    class Refusing:
        def bam_depth_device(self, native, tids, *a):
            calls.append(len(tids))
            if len(tids) > 8:
                raise L.VaporHipError(-4, "vapor_bam_depth_device: more than 1.5 GB of blocks in one call (use smaller batches)")
            return eng.bam_depth_device(native, tids, *a)
    monkeypatch.setenv("VAPOR_BAM_DEVICE_BATCH_MB", "8")
    be = seqio.InProcessBam()
    assert be.depth_many(Refusing(), path, ["c"] * 300, bounds) == host
    big, small = [c for c in calls if c > 8], [c for c in calls if c <= 8]
    assert len(big) >= 10 and sum(small) == 300 and max(calls) < 100
    # the calls themselves, in order: the groups of 8 MB as the index gives them, a refused one followed at once by its halves
    # (and a half that is refused again by its own)
    assert calls == [
        10, 5, 5, 10, 5, 5, 11, 5, 6, 15, 7, 8, 12, 6, 6, 10, 5, 5, 13, 6, 7, 8, 11, 5, 6, 8, 11, 5, 6, 10, 5, 5, 12, 6, 6,
        11, 5, 6, 12, 6, 6, 8, 9, 4, 5, 11, 5, 6, 11, 5, 6, 12, 6, 6, 10, 5, 5, 11, 5, 6, 12, 6, 6, 11, 5, 6, 10, 5, 5, 11, 5,
        6, 9, 4, 5, 10, 5, 5, 1]
    calls.clear()
    monkeypatch.setenv("VAPOR_BAM_DEVICE_BATCH_MB", "192")
    assert be.depth_many(eng, path, ["c"] * 300 + ["nowhere"], bounds + [(0, 1, 2, 3)]) == host + [[0, 0, 0]]
    monkeypatch.setenv("VAPOR_BAM_DEVICE", "0")
    assert be.depth_many(eng, path, ["c"] * 300, bounds) == host


def test_a_damaged_block_sends_its_regions_to_the_host_route_and_no_other(eng, many, tmp_path):
    good, bounds = many
    raw = bytearray(open(good, "rb").read())
    bl = TB._blocks(bytes(raw))
    off, bsize, _xlen = bl[len(bl) // 2]
    raw[off + bsize - 8] ^= 0x40                     # the block's CRC
    bad = str(tmp_path / "bad.bam")
    open(bad, "wb").write(bytes(raw))
    shutil.copy(good + ".bai", bad + ".bai")
    b = bamio.BamFile(bad)
    g = bamio.BamFile(good)
    cov, status, chunks = device(eng, b, ["c"] * 300, bounds)
    n_bad = 0
    for k, bd in enumerate(bounds):
        # a region touches the block iff one of its chunks' file ranges holds the block's offset
        touches = any((cs >> 16) <= off and (off < (ce >> 16) or (off == (ce >> 16) and (ce & 0xFFFF))) for cs, ce in chunks[k])
        assert status[k] == (REG_BLOCK if touches else 0), (k, status[k], touches)
        if touches:
            n_bad += 1
            assert cov[k] == [0, 0, 0]
            with pytest.raises(ValueError):          # the host route's answer for such a region: the file is damaged
                b.depth_native(0, bd)
        else:
            assert cov[k] == g.depth_native(0, bd) == b.depth_native(0, bd)
    assert 1 <= n_bad < 150, n_bad
    # depth_many hands the region to the host route, which words the error
    be = seqio.InProcessBam()
    with pytest.raises(ValueError, match="vapor_bam_depth"):
        be.depth_many(eng, bad, ["c"] * 300, bounds)
    ok = [k for k in range(300) if status[k] == 0]
    assert be.depth_many(eng, bad, ["c"] * len(ok), [bounds[k] for k in ok]) == [cov[k] for k in ok]
    b.close()
    g.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the CLI from files
# ------------------------------------------------------------------------------------------------------------------------------
def _run(tmp_path, name, cmd, text, fa, bam, more=()):
    d = tmp_path / name
    d.mkdir()
    src = d / ("in." + cmd)
    src.write_text(text)
    out = d / "out.vapor"
    from vapor_amd import simple_function as SF
    seen = {}
    orig = SF.vcf_vapor_modify

    def keep_table(vcf_input, rec_new, *a, **k):
        seen["table"] = open(vcf_input + ".vapor").read()
        return orig(vcf_input, rec_new, *a, **k)
    SF.vcf_vapor_modify = keep_table
    try:
        assert cli.main([cmd, "--sv-input", str(src), "--reference", fa, "--pacbio-input", bam, "--output-path", str(d / "figs"),
                         "--output-file", str(out), "--no-figures"] + list(more)) == 0
    finally:
        SF.vcf_vapor_modify = orig
    return seen["table"] if cmd == "vcf" else out.read_text()


@pytest.mark.parametrize("cmd", ["bed", "vcf"])
def test_cli_from_files_equals_the_host_routes_and_keeps_the_plain_columns(cmd, tmp_path, monkeypatch):
    specs = tuple(synth.DEPTH_SPECS) + (("DEL", 800, "het"), ("DEL", 300, "hom"), ("TANDUP", 500, "het"), ("DEL", 1100, "het"),
                                        ("DEL", 450, "het"), ("DEL", 2500, "hom"))
    w = synth.make_depth_world(seed=21, specs=specs, layers=3, read_len=1500, errors=(0.01, 0.03, 0.03))
    fa, bam = synth.write_world_files(w, str(tmp_path), block_size=8192)
    text = synth.bed_text(w) if cmd == "bed" else synth.vcf_text(w)
    seqio.set_backend(None)
    pipeline.set_engine(None)
    calls = []
    orig = Engine.bam_depth_device
    monkeypatch.setattr(Engine, "bam_depth_device", lambda self, *a, **k: calls.append(len(a[1])) or orig(self, *a, **k))
    try:
        table = _run(tmp_path, "dev", cmd, text, fa, bam, ["--depth"])
        n_dev = sum(calls)
        plain = _run(tmp_path, "plain", cmd, text, fa, bam)
        monkeypatch.setenv("VAPOR_BAM_DEVICE", "0")
        seqio.set_backend(None)
        calls.clear()
        host = _run(tmp_path, "host", cmd, text, fa, bam, ["--depth"])
        assert not calls
        monkeypatch.delenv("VAPOR_BAM_DEVICE")
        monkeypatch.setenv("VAPOR_BAM_NATIVE", "0")
        seqio.set_backend(None)
        py = _run(tmp_path, "py", cmd, text, fa, bam, ["--depth"])
        assert not calls
    finally:
        monkeypatch.delenv("VAPOR_BAM_NATIVE", raising=False)
        seqio.set_backend(None)
        pipeline.set_engine(None)
    assert table == host == py
    rows = [r.split("\t") for r in table.splitlines()]
    assert ["\t".join(r[:-4]) for r in rows] == plain.splitlines()
    measured = [r for r in rows[1:] if r[-4] != "."]
    n_loci = sum(l.svtype in ("DEL", "TANDUP") for l in w.loci) if cmd == "bed" else sum(l.svtype == "DEL" for l in w.loci)
    assert len(measured) == n_loci and n_dev >= n_loci             # (a locus above 2 P is two regions)
    # and the numbers are the world's, read with errors: deletions well below the flanks, duplications well above
    in_mem = seqio.MemorySamtools(w)
    by_contig = {(r[0] if cmd == "bed" else r[0].split(":")[0]): r for r in rows[1:]}
    assert len(by_contig) == len(rows) - 1 == (len(w.loci) if cmd == "bed" else sum(l.svtype != "TANDUP" for l in w.loci))
    for l in w.loci:
        if l.chrom not in by_contig:
            continue
        r = by_contig[l.chrom]
        regs = depth.regions(l.svtype, [l.chrom, l.start, l.end], len(w.contigs[l.chrom]))
        p = depth.payload(l.svtype, regs, in_mem.depth_many(None, "x", [l.chrom] * len(regs), regs))
        assert r[-4:] == depth.fold(l.svtype, p), l
        if l.svtype != "INV":
            assert r[-1] == "1"

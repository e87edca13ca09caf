"""Split reads joined through their SA tags on the device (`--links`, DESIGN.md 4.21: vapor_bam_links_device - bgzf_inflate_kernel,
bam_link_kernel) against the native host reader (vapor_bam_links), the Python statement (links.answer over bamio's records) and
the brute force of tests/links_cases.py: per region the five words and the status, exactly - one region per way the kernel can
go wrong (the designed file of links_cases.py, written once with blocks so small that record headers and SA values cross them
and once with large ones), 300 regions in one call and split over many, a file with a damaged block (a handled status), and the
CLI's tables from files."""
import shutil

import numpy as np
import pytest

import links_cases as LC
import test_bamio as TB
import test_gpu_depth as GD
import test_links_cpu as LK
import test_signature_cpu as SC
from vapor_amd import _lib as L
from vapor_amd import bamio, links, pipeline, seqio, synth
from vapor_amd.engine import Engine

pytestmark = pytest.mark.gpu

REG_MALFORMED, REG_BLOCK = 2, 5
T, C, Q = LC.T, LC.C, LC.Q
BLOCK = 1000


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def device(eng, b, cases):
    """engine.bam_links_device over the cases' .bai chunks: (five words per region, status per region, chunks per region)."""
    tids, rows, names, chunk_first, flat, per = LC.device_rows(b, cases)
    with b.handle(L.load()) as tl:
        out, status = eng.bam_links_device(tl["native"], tids, rows, chunk_first, flat, names)
    return [[int(x) for x in o] for o in out], status.tolist(), per


def host(b, case):
    _name, chrom, f, partner, _e, _s = case
    return b.links_native(b.tid[chrom], list(f) + [0, len(partner)], None, partner)


def statement(b, case, min_mapq=0):
    _name, chrom, f, partner, _e, _s = case
    recs = b.fetch_links(chrom, int(f[0]) + 1, int(f[1]), exclude_more=links.EXCLUDE) if f[1] > f[0] else []
    return links.words(links.answer(recs, f, partner, min_mapq))


@pytest.fixture(scope="module", params=[BLOCK, 0xFF00])
def designed(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gpu_links") / ("designed_%d.bam" % request.param))
    return path, LC.write_designed(path, request.param), request.param


def test_every_designed_region_equals_host_statement_and_model(eng, designed):
    path, d, block = designed
    b = bamio.BamFile(path)
    out, status, chunks = device(eng, b, d.cases)
    by_name = {}
    for case, got, st, ch in zip(d.cases, out, status, chunks):
        name, chrom, f, partner, expect, want_status = case
        want = LC.brute(d.recs[b.tid[chrom]], f, partner)
        assert st == want_status, (name, st)
        assert host(b, case) == want == statement(b, case) and (expect is None or want == expect), (name, want, expect)
        # a region the device hands back has no words; the host's answer stands
        assert got == (want if st == 0 else [0] * 5), (name, got, want)
        by_name[name] = (got, ch)
    # the properties the cases are there for, beside their expected words
    assert sum(st == REG_MALFORMED for st in status) == 2 and sum(st != 0 for st in status) == 2
    assert len(by_name["two .bai chunks"][1]) >= 2 and by_name["an empty window"][1] == []
    assert all(by_name["rname of %d bytes" % n][0] == [1, 1, 1, n % 5, 1] for n in range(1, 72))
    assert by_name["an entry below the cut"][0] == [2, 2, 2, 0, 1]
    if block == BLOCK:
        # a record header and an SA value across two BGZF blocks are among the records walked
        starts = dict((name, q) for q, name in GD._record_starts(path))
        crossing = [name for name, q in starts.items() if q // block != (q + 35) // block]
        assert len(crossing) > 3
        row = {r[0]: r for r in d.rows}["n40_last"]
        q = starts["n40_last"]
        lo = q + 4 + 32 + len("n40_last") + 1 + 4 * 2 + (140 + 1) // 2 + 140 + 3
        assert lo // block != (lo + len(row[5]) - 4) // block and len(row[5]) > 1000
    b.close()


def test_with_the_handles_filter(eng, designed):
    path, d, _block = designed
    b = bamio.BamFile(path)
    cases = [c for c in d.cases if c[0] in ("an entry below the cut", "records that never count, and the user's filter", "SA as the first aux field",
                                            "rel same, FLAG 0x10 on and off")]
    seen = []
    for flt in ((0, 0), (0, 0x800), (Q, 0), (Q, 0x810)):
        b.set_filter(*flt)
        out, status, _ = device(eng, b, cases)
        assert status == [0] * len(cases)
        for case, got in zip(cases, out):
            assert got == host(b, case) == LC.brute(d.recs[0], case[2], case[3], flt) == statement(b, case, flt[0]), (case[0], flt)
        by = {c[0]: g for c, g in zip(cases, out)}
        seen.append((by["an entry below the cut"], by["records that never count, and the user's filter"][0]))
    assert seen == [([2, 2, 2, 0, 1], 5), ([2, 2, 2, 0, 1], 4), ([2, 1, 1, 4, 1], 4), ([2, 1, 1, 4, 1], 2)]
    b.set_filter(0, 0)
    b.set_dedup(True)
    assert device(eng, b, cases)[0] == [LC.brute(d.recs[0], c[2], c[3]) for c in cases]      # --dedup-qname has no effect
    b.close()


def test_refused_regions_and_arguments(eng, designed):
    path, d, _block = designed
    b = bamio.BamFile(path)
    with b.handle(L.load()) as tl:
        case = d.cases[0]
        f = case[2]
        ch = np.asarray(b.index.chunks(0, f[0], f[1]), dtype=np.uint64).reshape(-1)
        names = b"xx" + case[3]
        good = tuple(f) + (2, len(case[3]))
        bad = [good[:k] + (v,) + good[k + 1:] for k, v in ((0, f[1] + 1), (1, 1 << 31), (4, -1), (4, 256), (6, 2), (7, -1), (8, 2), (10, 0), (10, len(names)), (9, -1), (0, -1))]
        regions = np.asarray([good] + bad + [good], dtype=np.int64)
        n = len(regions)
        first = np.arange(n + 1, dtype=np.int32) * (len(ch) // 2)
        out, status = eng.bam_links_device(tl["native"], [0] * (n - 1) + [-1], regions, first, np.tile(ch, n), names)
        assert status.tolist() == [0] + [REG_MALFORMED] * (n - 1) and out[1:].tolist() == [[0] * 5] * (n - 1) and out[0].tolist() == case[4] == [1, 1, 1, 0, 1]
        out, status = eng.bam_links_device(tl["native"], [], np.zeros((0, 11), dtype=np.int64), [0], [], b"")
        assert len(out) == 0 and len(status) == 0
        # a call without names: every region is refused by status, nothing is read
        out, status = eng.bam_links_device(tl["native"], [0], np.asarray([good], dtype=np.int64), first[:2], ch, b"")
        assert status.tolist() == [REG_MALFORMED] and out.tolist() == [[0] * 5]
    b.close()


# ------------------------------------------------------------------------------------------------------------------------------
# many regions
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many(tmp_path_factory):
    rows, recs, cases = LC.seeded_world(np.random.default_rng(12))
    path = str(tmp_path_factory.mktemp("gpu_links_many") / "many.bam")
    bamio.write_bam(path, [("c", 60000)], rows, block_size=20000)
    return path, cases, recs


def args_of(cases):
    return [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases]


def test_300_regions_in_one_call_and_split_and_halved(eng, many, monkeypatch):
    path, cases, recs = many
    b = bamio.BamFile(path)
    out, status, chunks = device(eng, b, cases)
    assert status == [0] * 300
    want = [host(b, c) for c in cases]
    assert out == want
    for g in range(0, 300, 3):
        assert out[g] == statement(b, cases[g]) == LC.brute(recs, cases[g][2], cases[g][3])
    assert sum(o[0] > 0 for o in out) > 100 and sum(o[2] > 0 for o in out) > 30 and sum(o[1] > o[2] for o in out) > 30 and sum(o[4] > 1 for o in out) > 5
    b.close()
    # the same through links_many, its groups so small that the call is split, and a library that refuses more than 8 regions
    # "in one call" so that the groups are halved
    calls = []

    class Refusing:
        def bam_links_device(self, native, tids, *a, **k):
            calls.append(len(tids))
            if len(tids) > 8:
                raise L.VaporHipError(-4, "vapor_bam_links_device: more than 1.5 GB of blocks in one call (use smaller batches)")
            return eng.bam_links_device(native, tids, *a, **k)
    monkeypatch.setenv("VAPOR_BAM_DEVICE_BATCH_MB", "8")
    be = seqio.InProcessBam()
    assert be.links_many(Refusing(), path, *args_of(cases)) == want
    big, small = [c for c in calls if c > 8], [c for c in calls if c <= 8]
    assert len(big) >= 3 and sum(small) == 300 and max(calls) < 300
    # the calls themselves, in order: the groups of 8 MB as the index gives them, a refused one followed at once by its halves
    # (and a half that is refused again by its own)
    assert calls == [
        15, 7, 8, 18, 9, 4, 5, 9, 4, 5, 18, 9, 4, 5, 9, 4, 5, 19, 9, 4, 5, 10, 5, 5, 19, 9, 4, 5, 10, 5, 5, 18, 9, 4, 5, 9, 4,
        5, 18, 9, 4, 5, 9, 4, 5, 16, 8, 8, 17, 8, 9, 4, 5, 17, 8, 9, 4, 5, 19, 9, 4, 5, 10, 5, 5, 16, 8, 8, 16, 8, 8, 17, 8,
        9, 4, 5, 17, 8, 9, 4, 5, 17, 8, 9, 4, 5, 16, 8, 8, 7]
    calls.clear()
    monkeypatch.setenv("VAPOR_BAM_DEVICE_BATCH_MB", "192")
    more = cases + [("nowhere", "nowhere", (0, 30, 10, 20, 5, C, 0, 0, 0), b"c", None, 0)]
    assert be.links_many(eng, path, *args_of(more)) == want + [[0] * 5]
    monkeypatch.setenv("VAPOR_BAM_DEVICE", "0")
    assert be.links_many(eng, path, *args_of(cases)) == want
    # under the filter, entries' mapQ included
    monkeypatch.delenv("VAPOR_BAM_DEVICE")
    be.read_filter = (Q, 0x800)
    got = be.links_many(eng, path, *args_of(cases))
    assert got == [LC.brute(recs, c[2], c[3], (Q, 0x800)) for c in cases] and got != want


def test_a_malformed_aux_area_goes_to_the_host_through_links_many(eng, designed):
    path, d, _block = designed
    be = seqio.InProcessBam()
    calls = []

    class Counting:
        def bam_links_device(self, native, tids, *a, **k):
            out, status = eng.bam_links_device(native, tids, *a, **k)
            calls.append(status.tolist())
            return out, status
    got = be.links_many(Counting(), path, *args_of(d.cases))
    assert got == [LC.brute(d.recs[{"c": 0, "d": 1}[c[1]]], c[2], c[3]) for c in d.cases]
    assert sum(st == REG_MALFORMED for call in calls for st in call) == 2 and sum(st != 0 for call in calls for st in call) == 2


def test_a_damaged_block_sends_its_regions_to_the_host_route_and_no_other(eng, many, tmp_path):
    good, cases, _recs = many
    raw = bytearray(open(good, "rb").read())
    bl = TB._blocks(bytes(raw))
    off, bsize, _xlen = bl[len(bl) // 2]
    raw[off + bsize - 8] ^= 0x40                     # the block's CRC
    bad = str(tmp_path / "bad.bam")
    open(bad, "wb").write(bytes(raw))
    shutil.copy(good + ".bai", bad + ".bai")
    b = bamio.BamFile(bad)
    g = bamio.BamFile(good)
    out, status, chunks = device(eng, b, cases)
    n_bad = 0
    for k, case in enumerate(cases):
        # a region touches the block iff one of its chunks' file ranges holds the block's offset
        touches = any((cs >> 16) <= off and (off < (ce >> 16) or (off == (ce >> 16) and (ce & 0xFFFF))) for cs, ce in chunks[k])
        assert status[k] == (REG_BLOCK if touches else 0), (k, status[k], touches)
        if touches:
            n_bad += 1
            assert out[k] == [0] * 5
            with pytest.raises(ValueError):          # the host route's answer for such a region: the file is damaged
                host(b, case)
        else:
            assert out[k] == host(g, case) == host(b, case)
    assert 1 <= n_bad < 250, n_bad
    # links_many hands the region to the host route, which words the error
    be = seqio.InProcessBam()
    with pytest.raises(ValueError, match="vapor_bam_links"):
        be.links_many(eng, bad, *args_of(cases))
    ok = [k for k in range(300) if status[k] == 0]
    if ok:
        assert be.links_many(eng, bad, *args_of([cases[k] for k in ok])) == [out[k] for k in ok]
    b.close()
    g.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the CLI from files
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cmd", ["bed", "vcf"])
def test_cli_from_files_equals_the_host_routes_and_the_closed_form(cmd, tmp_path, monkeypatch):
    w = synth.make_links_world(seed=21, reads=LK.READS, jitter=LK.JITTER)
    expect = LK.closed_form(w)
    fa, bam = synth.write_world_files(w, str(tmp_path), block_size=8192)
    text = synth.bed_text(w) if cmd == "bed" else synth.links_vcf_text(w)
    opts = ["--links"] + (["--bnd"] if cmd == "vcf" else [])
    seqio.set_backend(None)
    pipeline.set_engine(None)
    calls = []
    orig = Engine.bam_links_device
    monkeypatch.setattr(Engine, "bam_links_device", lambda self, *a, **k: calls.append(len(a[1])) or orig(self, *a, **k))
    try:
        table, _ = SC.run_main(tmp_path, "dev", cmd, text, opts, fa, bam)
        n_dev = sum(calls)
        plain, _ = SC.run_main(tmp_path, "plain", cmd, text, opts[1:], fa, bam)
        monkeypatch.setenv("VAPOR_BAM_DEVICE", "0")
        seqio.set_backend(None)
        calls.clear()
        host_table, _ = SC.run_main(tmp_path, "host", cmd, text, opts, fa, bam)
        assert not calls
        monkeypatch.delenv("VAPOR_BAM_DEVICE")
        monkeypatch.setenv("VAPOR_BAM_NATIVE", "0")
        seqio.set_backend(None)
        py, _ = SC.run_main(tmp_path, "py", cmd, text, opts, fa, bam)
        assert not calls
    finally:
        monkeypatch.delenv("VAPOR_BAM_NATIVE", raising=False)
        seqio.set_backend(None)
        pipeline.set_engine(None)
    assert table == host_table == py
    rows = LK.columns_of(table)
    assert "\n".join("\t".join(r[:-7]) for r in rows) + "\n" == plain
    by_contig = {(r[0] if cmd == "bed" else r[0].split(":")[0]): r[-7:] for r in rows[1:]}
    n_loci = n_regions = 0
    for l, e in zip(w.loci, expect):
        if (cmd == "vcf" and l.svtype == "TANDUP") or (cmd == "bed" and l.svtype == "BND"):
            continue
        n_loci += 1
        n_regions += 4 if l.svtype == "INV" else 2
        assert by_contig[l.chrom] == e, (l, by_contig[l.chrom], e)
    assert len(by_contig) == n_loci and n_dev == n_regions

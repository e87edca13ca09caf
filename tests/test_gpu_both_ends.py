"""`--both-ends` on the device: the right-anchored chop kernel (vapor_bam_chop_device_right:
bam_chop_right_kernel) against the host reader's (vapor_bam_chop_right, itself pinned on the Python statement and its definition
in tests/test_both_ends_cpu.py) per region - count, q1, miss_bp and the bases, as the bit planes of a set made from the device
addresses with src_kind 2 against those of the same reverse-complemented text uploaded as bytes; a damaged block; and the
command line from memory and from files against the run of the same command with the CPU test's stand-in engine."""
import os
import shutil

import numpy as np
import pytest

import test_bamio as TB
import test_both_ends_cpu as C
from vapor_amd import _lib as L
from vapor_amd import bamio, cli, drivers, pipeline, seqio, synth
from vapor_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture()
def clean_state():
    pipeline.set_engine(None)
    yield
    pipeline.set_engine(None)
    seqio.set_backend(None)


def compare_right(eng, bam, regions, max_keep=20):
    """regions: (chrom, start, end, flank).  The device's status per region; for every region it answered, the kept reads are
    the host's: their number, miss_bp, q1 (through the bases) and the reverse-complemented bases themselves."""
    be = seqio.InProcessBam()
    b = be._open(bam)
    chroms = [r[0] for r in regions]
    st = np.asarray([r[1] for r in regions], dtype=np.int64)
    en = np.asarray([r[2] for r in regions], dtype=np.int64)
    fl = np.asarray([r[3] for r in regions], dtype=np.int64)
    dkf, daddr, dq1, dmiss, dstatus, batches = be.chop_many_device(eng, bam, chroms, st, en, fl, max_keep, right=True)
    texts, lens, sel = [], [], []
    try:
        for g in range(len(regions)):
            if dstatus[g]:
                continue
            r = b.chop_native_raw(chroms[g], int(st[g]), int(en[g]), int(fl[g]), right=True)
            a, e = int(dkf[g]), int(dkf[g + 1])
            if r is None:
                assert e == a, g
                continue
            whole, off, ln, miss = r
            order = np.arange(len(off))
            if len(order) > max_keep:
                order = np.argsort(miss, kind="stable")[:max_keep]
            assert e - a == len(order) and dmiss[a:e].tolist() == miss[order].tolist(), (g, regions[g])
            for t, i in enumerate(order):
                assert int(ln[i]) == int(en[g] - st[g] - miss[i])
                assert int(dq1[a + t]) + 1 >= int(ln[i])
                texts.append(whole[int(off[i]):int(off[i]) + int(ln[i])])
                lens.append(int(ln[i]))
                sel.append(a + t)
        if texts:
            sel = np.asarray(sel)
            dev = eng.seqset_raw(daddr[sel], np.asarray(lens, dtype=np.int64), None, src_kind=np.full(len(sel), 2, dtype=np.uint8), src_first=dq1[sel])
            ref = eng.seqset(texts)
            try:
                for t in range(len(texts)):
                    assert all(np.array_equal(x, y) for x, y in zip(dev.planes(t), ref.planes(t))), t
                assert np.array_equal(dev.n_exc, ref.n_exc) and np.array_equal(dev.n_invalid, ref.n_invalid)
            finally:
                dev.close()
                ref.close()
    finally:
        for bt in batches:
            bt.close()
        b.close()
    return dstatus, len(texts)


def _worlds():
    w = C._mixed_world()
    for c in w.reads:
        w.reads[c] = sorted(w.reads[c], key=lambda r: r.pos)
    return w


def _view_regions(w):
    """The window of every view of every junction locus of the world (L and R alike: the right-anchored chop of each)."""
    regions = []
    for l in w.loci:
        if l.svtype == "BND":
            for c, x in ((l.chrom, l.start), (l.extra["mate_chrom"], l.end), (l.extra["mate_chrom"], l.end - 1)):
                regions.append((c, x - 500, x + 500, 500))
        elif l.end - l.start >= 10000:
            regions += [(l.chrom, l.start - 500, l.start + 500, 500), (l.chrom, l.end - 500, l.end + 500, 500)]
    return regions


def test_device_chop_equals_host_chop_on_world_files(eng, tmp_path):
    w = _worlds()
    regions = _view_regions(w) + [("no_such_contig", 5, 900, 100), (w.loci[0].chrom, 1, 40, 10), (w.loci[0].chrom, 100, 3000, 1500)]
    for block in (0xFF00, 1500):
        d = tmp_path / ("b%d" % block)
        d.mkdir()
        fa, bam = synth.write_world_files(w, str(d), block_size=block)
        status, n = compare_right(eng, bam, regions)
        assert status.tolist() == [0] * len(regions) and n > 80, (block, status.tolist(), n)


def test_long_cigar_in_the_cg_tag_and_every_operation(eng, tmp_path):
    rng = np.random.default_rng(33)
    refs = [("chrA", 200000), ("chrB", 90000)]
    reads = []
    for i in range(60):
        tid = int(rng.integers(0, 2)); pos = int(rng.integers(0, 60000))
        ops, seq_len = [], 0
        for _ in range(int(rng.integers(1, 30))):
            o = "MIDS=XN"[int(rng.integers(0, 7))]; n = int(rng.integers(1, 400))
            ops.append((n, o)); seq_len += n if o in "MIS=X" else 0
        if seq_len == 0:
            ops.append((5, "M")); seq_len = 5
        seq = "".join("ACGTNRYK"[j] for j in rng.integers(0, 8, seq_len))
        reads.append(("q%d" % i, tid, pos, ops, seq, b"NMC\x05RGZgrp1\0" if i % 2 else b""))
    n_ops = 70000                          # beyond the 65 535 operations a record's own field holds: CG:B,I
    reads.append(("qlong", 0, 1000, [(1, "M") if j % 2 == 0 else (1, "I") for j in range(n_ops)], "ACGT" * (n_ops // 4), b"NMC\x01"))
    reads.append(("qlong2", 0, 2000, [(3, "S")] + [(2, "M") if j % 2 == 0 else (1, "D") for j in range(n_ops)] + [(40, "S")],
                  "ACGTG" * ((3 + n_ops + 40) // 5 + 1), b""))
    reads[-1] = reads[-1][:4] + (reads[-1][4][:3 + n_ops + 40],) + reads[-1][5:]
    reads.sort(key=lambda r: (r[1] if r[1] >= 0 else 1 << 30, r[2]))
    p = str(tmp_path / "ind.bam")
    TB._encode_bam(p, refs, reads)
    regions = [("chrA", 35200, 35900, 300), ("chrA", 20000, 26000, 500), ("chrB", 5000, 9000, 500), ("chrA", 1, 100000, 500),
               ("chrB", 30000, 30100, 40), ("chrA", 35990, 36001, 20), ("chrZ", 1, 10, 5), ("chrA", 1100, 30000, 300),
               ("chrA", 100000, 106000, 1000), ("chrA", 104000, 106999, 400), ("chrA", 106500, 107001, 100)]
    status, n = compare_right(eng, p, regions)
    assert status.tolist() == [0] * len(regions) and n >= 4, (status.tolist(), n)


def test_more_candidates_than_are_kept(eng, tmp_path):
    rng = np.random.default_rng(9)
    contig = synth.random_dna(rng, 60000)
    recs = []
    for i in range(90):
        pos = 4000 + int(rng.integers(0, 900))
        post = int(rng.integers(0, 40))
        read, cg = synth.mutate(rng, contig[pos:pos + 6000])
        recs.append(("m%d" % i, 0, pos, cg + "%dD" % int(rng.integers(1, 700)) + "5M" + ("%dS" % post if post else ""), read + "ACGTA" + synth.random_dna(rng, post)))
    recs.sort(key=lambda r: r[2])
    p = str(tmp_path / "many.bam")
    bamio.write_bam(p, [("c", 60000)], recs, block_size=0xFF00)
    status, n = compare_right(eng, p, [("c", 9000, 10400, 1000), ("c", 9500, 10300, 1400)])
    assert status.tolist() == [0, 0] and n == 40


def test_a_damaged_block_sends_its_regions_to_the_host_route_and_no_other(eng, tmp_path):
    rng = np.random.default_rng(5)
    contig = synth.random_dna(rng, 400000)
    recs = []
    for i in range(160):
        pos = 2000 * i + int(rng.integers(0, 500))
        read, cg = synth.mutate(rng, contig[pos:pos + 5000])
        recs.append(("m%d" % i, 0, pos, cg, read))
    good = str(tmp_path / "good.bam")
    bamio.write_bam(good, [("c", 400000)], recs, block_size=20000)
    raw = bytearray(open(good, "rb").read())
    bl = TB._blocks(bytes(raw))
    off, bsize, xlen = bl[len(bl) // 2]
    raw[off + bsize - 8] ^= 0x40                                   # the block's CRC
    bad = str(tmp_path / "bad.bam")
    open(bad, "wb").write(bytes(raw))
    shutil.copy(good + ".bai", bad + ".bai")
    regions = [("c", 2000 * i + 3600, 2000 * i + 4500, 300) for i in range(4, 150, 3)]
    be = seqio.InProcessBam()
    st = np.asarray([r[1] for r in regions]); en = np.asarray([r[2] for r in regions]); fl = np.asarray([r[3] for r in regions])
    dkf, daddr, dq1, dmiss, dstatus, batches = be.chop_many_device(eng, bad, ["c"] * len(regions), st, en, fl, right=True)
    for bt in batches:
        bt.close()
    # every region the device answered: count, miss_bp and bases are the host reader's, on the damaged file
    st2, n_cmp = compare_right(eng, bad, regions)
    assert st2.tolist() == dstatus.tolist() and n_cmp > 50
    b, bg = be._open(bad), be._open(good)
    n_bad = n_reads = 0
    for g, r in enumerate(regions):
        want = bg.chop_native(*r, right=True)                      # (the host route of the undamaged file: the same reads)
        try:
            host = b.chop_native(*r, right=True)
            assert host == want
            assert dstatus[g] == 0 and int(dkf[g + 1] - dkf[g]) == min(len(host), 20), (g, dstatus[g])
            n_reads += len(host)
        except ValueError:
            n_bad += 1
            assert dstatus[g] != 0, g                              # (what the host refuses, the device has not answered)
    assert 1 <= n_bad <= 12 and (dstatus != 0).sum() == n_bad and n_reads > 50


def test_planes_of_a_reverse_complemented_device_source(eng, tmp_path):
    """vapor_seqset_planes of a src_kind 2 sequence = the planes of the same rc text uploaded as bytes: lengths that are no
    multiple of 32, odd and even first bases, the first base of the read, one base; a source that would start before its read's
    first base or outside the batch is refused."""
    rng = np.random.default_rng(12)
    seq = "".join("=ACMGRSVTWYHKDBN"[j] for j in rng.integers(0, 16, 3001))
    p = str(tmp_path / "one.bam")
    bamio.write_bam(p, [("c", 9000)], [("r", 0, 100, "3001M", seq)])
    be = seqio.InProcessBam()
    kf, addr, q0, miss, status, batches = be.chop_many_device(eng, p, ["c"], [101], [700], [100])
    try:
        assert int(kf[-1]) == 1 and int(q0[0]) == 0 and status.tolist() == [0]
        cases = [(0, 1), (1, 1), (1, 2), (31, 32), (32, 33), (63, 64), (64, 33), (999, 1000), (1000, 1000), (2999, 777), (3000, 3001),
                 (3000, 31), (2001, 1025), (2002, 1025)]
        firsts = np.asarray([c[0] for c in cases], dtype=np.int64)
        lens = np.asarray([c[1] for c in cases], dtype=np.int64)
        a = np.full(len(cases), addr[0], dtype=np.uint64)
        dev = eng.seqset_raw(a, lens, None, src_kind=np.full(len(cases), 2, dtype=np.uint8), src_first=firsts)
        ref = eng.seqset([seqio.rc_read(seq[f - n + 1:f + 1]) for f, n in cases])
        try:
            for t in range(len(cases)):
                assert all(np.array_equal(x, y) for x, y in zip(dev.planes(t), ref.planes(t))), cases[t]
            assert np.array_equal(dev.n_exc, ref.n_exc) and np.array_equal(dev.n_invalid, ref.n_invalid)
        finally:
            dev.close()
            ref.close()
        # forward and reverse sources in one set, with a host sequence between them
        mix = eng.seqset_raw(np.asarray([addr[0], 0, addr[0]], dtype=np.uint64), np.asarray([100, 0, 100], dtype=np.int64), None,
                             src_kind=np.asarray([1, 0, 2], dtype=np.uint8), src_first=np.asarray([7, 0, 106], dtype=np.int64))
        r2 = eng.seqset([seq[7:107], "", seqio.rc_read(seq[7:107])])
        try:
            for t in (0, 2):
                assert all(np.array_equal(x, y) for x, y in zip(mix.planes(t), r2.planes(t))), t
        finally:
            mix.close()
            r2.close()
        one = np.asarray([2], dtype=np.uint8)
        with pytest.raises(L.VaporHipError):                       # more bases than lie before the first one
            eng.seqset_raw(addr[:1], np.asarray([12], dtype=np.int64), None, src_kind=one, src_first=np.asarray([10], dtype=np.int64))
        with pytest.raises(L.VaporHipError):
            eng.seqset_raw(addr[:1], np.asarray([5], dtype=np.int64), None, src_kind=np.asarray([3], dtype=np.uint8), src_first=np.asarray([10], dtype=np.int64))
    finally:
        for bt in batches:
            bt.close()
    with pytest.raises(L.VaporHipError):                           # the batch is gone
        eng.seqset_raw(addr[:1], np.asarray([5], dtype=np.int64), None, src_kind=np.asarray([2], dtype=np.uint8), src_first=np.asarray([10], dtype=np.int64))


def _tables(tmp_path, name, w, ref, bam):
    vt, vf = C._main(tmp_path, name + "_vcf", "vcf", C._mixed_vcf(w), ["--both-ends"])
    bt, _ = C._main(tmp_path, name + "_bed", "bed", synth.bed_text(w), ["--both-ends"])
    return vt, vf, bt


def _main_files(tmp_path, name, mode, text, ref, bam):
    d = tmp_path / name
    d.mkdir()
    src = d / ("in." + mode)
    src.write_text(text)
    out = d / "out.vapor"
    args = [mode, "--sv-input", str(src), "--reference", ref, "--pacbio-input", bam, "--output-path", str(d / "figs"),
            "--output-file", str(out), "--no-figures", "--both-ends"] + (["--bnd"] if mode == "vcf" else [])
    assert cli.main(args) == 0
    return (d / "in.vcf.vapor").read_text() if mode == "vcf" else out.read_text()


def test_cli_tables_equal_the_cpu_run_from_memory_and_from_files(clean_state, oracle, tmp_path):
    """`vapor vcf --bnd --both-ends` and `vapor bed --both-ends` on the device: the table, the annotated VCF and the BED table
    are byte for byte those of the same run with the CPU test's stand-in engine - from the world in memory and from its FASTA
    and BAM files."""
    from fake_engine import FakeEngine
    w = _worlds()
    os.environ["VAPOR_QC_SEED"] = "7"
    try:
        pipeline.set_engine(FakeEngine(oracle))
        seqio.set_backend(seqio.MemorySamtools(w))
        cpu = _tables(tmp_path, "cpu", w, "ref.fa", "x.bam")
        pipeline.set_engine(None)
        seqio.set_backend(seqio.MemorySamtools(w))
        mem = _tables(tmp_path, "mem", w, "ref.fa", "x.bam")
        assert mem == cpu
        fd = tmp_path / "files"
        fd.mkdir()
        fa, bam = synth.write_world_files(w, str(fd))
        seqio.set_backend(seqio.InProcessBam())
        # from files every view's reads are selected on the device (seqio.prefetch_views: both chop kernels) and scored by
        # device address (src_kind 1 and 2): the windows asked for, the regions the library saw, no host chop of a BAM region
        asked, host_chops = [], []
        real_pre, real_chop = seqio.prefetch_views, seqio.InProcessBam.chop

        def spy_pre(engine, bam_name, windows, *a, **k):
            got = real_pre(engine, bam_name, windows, *a, **k)
            asked.append((len({x for x in windows if not x[4]}), len({x for x in windows if x[4]}), len(got.prefetched),
                          sum(len(v) for v in got.prefetched.values()), engine.bam_last_stats()["regions"]))
            return got

        def spy_chop(self, *a, **k):
            host_chops.append(a)
            return real_chop(self, *a, **k)
        seqio.prefetch_views, seqio.InProcessBam.chop = spy_pre, spy_chop
        try:
            assert _main_files(tmp_path, "f_vcf", "vcf", C._mixed_vcf(w), fa, bam) == cpu[1]
            assert _main_files(tmp_path, "f_bed", "bed", synth.bed_text(w), fa, bam) == cpu[2]
        finally:
            seqio.prefetch_views, seqio.InProcessBam.chop = real_pre, real_chop
        assert len(asked) == 2 and not host_chops
        for n_left, n_right, n_answered, n_reads, regions_seen in asked:
            assert n_left >= 5 and n_right >= 5 and n_answered == n_left + n_right and n_reads > 80 and regions_seen == n_right
    finally:
        os.environ.pop("VAPOR_QC_SEED", None)
    rows = [r.split("\t") for r in cpu[0].splitlines()[1:]]
    assert sum(1 for r in rows if r[6] == "2") >= 4 and any(r[6] == "4" for r in rows)


def test_mirror_equivalence_on_the_device(clean_state):
    """The R views of W on the device against the primary views of mirror_world(W) on the device."""
    W = synth.make_junction_world(C.JUNCTION_SEED)
    M = synth.mirror_world(W)
    fns = {"DEL": drivers.vapor_simple_del, "INV": drivers.vapor_simple_inv, "TANDUP": drivers.vapor_simple_tandup}
    seqio.set_backend(seqio.MemorySamtools(W))
    got = pipeline.run_batch([drivers.vapor_both_ends(l.svtype, 3, 1, "x.bam", "ref.fa", [l.chrom, l.start, l.end], "f.png") for l in W.loci])
    seqio.set_backend(seqio.MemorySamtools(M))
    exp = pipeline.run_batch([fns[m.svtype](3, 1, "x.bam", "ref.fa", [m.chrom, m.start, m.end], "f.png") for m in M.loci] +
                             [drivers.vapor_bnd(3, 1, "x.bam", "ref.fa", [m.chrom, m.end, m.chrom, m.start, "3to3", ""], "f.png")
                              for m in M.loci if m.svtype == "INV"])
    for g, e, l in zip(got, exp, W.loci):
        r = g.views[2] if l.svtype == "INV" else g.views[1]
        assert r and sorted(r) == sorted(e), l.svtype
    inv = [g for g, l in zip(got, W.loci) if l.svtype == "INV"][0]
    assert sorted(inv.views[3]) == sorted(exp[-1]) and len(exp[-1]) > 3
    Wb = synth.make_bnd_world(C.BND_SEED, forms=("3to5", "5to3", "5to5"), n_reads=12, ins=C.INS)
    Mb = synth.mirror_world(Wb)
    rw, rm = synth.bnd_records(Wb), synth.bnd_records(Mb)
    seqio.set_backend(seqio.MemorySamtools(Wb))
    got = pipeline.run_batch([drivers.vapor_both_ends("BND", 3, 1, "x.bam", "ref.fa", cli.bnd_view(r[0], int(r[1]), r[4], True), "f.png")
                              for r in rw[0::2]])
    seqio.set_backend(seqio.MemorySamtools(Mb))
    exp = pipeline.run_batch([drivers.vapor_bnd(3, 1, "x.bam", "ref.fa", cli.bnd_view(r[0], int(r[1]), r[4]), "f.png") for r in rm])
    assert sorted(got[0].views[1]) == sorted(exp[0]) and sorted(got[1].views[1]) == sorted(exp[2])
    assert sorted(got[2].views[0]) == sorted(exp[4]) and sorted(got[2].views[1]) == sorted(exp[5]) and len(exp[4]) > 3

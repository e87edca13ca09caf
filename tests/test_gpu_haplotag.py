"""`--phase-vcf` on the device (vapor_bam_chop_device_haplotag: bam_chop_ops_kernel, bam_haplotag_kernel, bam_select_kernel)
against the statement (phase.haplotag) and the host readers (vapor_bam_chop_haplotag + phase.select): the hand-written table of
tests/test_haplotag_cpu.py, the shapes at which the kernel's tiles end (65, 128 and 129 operations with a site in the operation at
each tile's lane 0 and lane 63; 63, 64 and 65 sites; a 70 001-operation CG record with sites near its end; a full slot; 64 phase
sets on the device and 65 on the host route; no site at all), the 12 x 30 world from files, the CLI tables of the device route,
the host-reader route, the drivers' route and the truth-tagged `--phased` run, and a file with a damaged block."""
import shutil

import numpy as np
import pytest

import test_bamio as TB
import test_haplotag_cpu as TC
from vapor_amd import bamio, cli, phase, pipeline, seqio, synth
from vapor_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def compare(eng, bam, regions, sites, max_keep=20, host_bam=None):
    """regions: (chrom, start, end, flank).  Returns the device's status per region, the reads compared, and per region it
    answered (tagged, P, member words, the host's (hap, ps) of the union's reads); for every such region the union, the member
    words, the phase set, miss_bp and the bases are the host's (of `host_bam`, the file itself unless given)."""
    be = seqio.InProcessBam()
    b = be._open(host_bam or bam)
    chroms = [r[0] for r in regions]
    st = np.asarray([r[1] for r in regions], dtype=np.int64)
    en = np.asarray([r[2] for r in regions], dtype=np.int64)
    fl = np.asarray([r[3] for r in regions], dtype=np.int64)
    dkf, daddr, dq0, dmiss, dstatus, batches, dmember, dps, dtagged = be.chop_many_device(eng, bam, chroms, st, en, fl, max_keep, groups=True,
                                                                                          sites=sites)
    texts, lens, sel, answers = [], [], [], {}
    try:
        for g in range(len(regions)):
            if dstatus[g]:
                continue
            r = b.chop_native_raw(chroms[g], int(st[g]), int(en[g]), int(fl[g]), tagged=True, sites=sites)
            a, e = int(dkf[g]), int(dkf[g + 1])
            if r is None:
                assert e == a and not dtagged[g] and dps[g] == phase.PS_NONE, g
                continue
            whole, off, ln, miss, hap, ps = r
            tagged, p, order, words = phase.select_numbers(miss, hap, ps, max_keep)
            assert (bool(dtagged[g]), int(dps[g])) == (tagged, p), (g, regions[g])
            assert e - a == len(order) <= 3 * max_keep and dmiss[a:e].tolist() == miss[order].tolist(), (g, regions[g])
            assert dmember[a:e].tolist() == words, (g, regions[g])
            answers[g] = (tagged, p, words, [(int(hap[i]), int(ps[i])) for i in order])
            for t, i in enumerate(order):
                texts.append(whole[int(off[i]):int(off[i]) + int(ln[i])])
                lens.append(int(ln[i]))
                sel.append(a + t)
        if texts:
            sel = np.asarray(sel)
            dev = eng.seqset_raw(daddr[sel], np.asarray(lens, dtype=np.int64), None, src_kind=np.ones(len(sel), dtype=np.uint8), src_first=dq0[sel])
            ref = eng.seqset(texts)
            try:
                for t in range(len(texts)):
                    assert all(np.array_equal(x, y) for x, y in zip(dev.planes(t), ref.planes(t))), t
            finally:
                dev.close()
                ref.close()
    finally:
        for bt in batches:
            bt.close()
        b.close()
    return dstatus, len(texts), answers


def one_read(answer):
    """(hap, ps) of the only kept read of a region, as the device's answer shows it: the read's group bits and the phase set."""
    tagged, p, words, _host = answer
    assert len(words) == 1
    hap = 1 if words[0] & 2 else 2 if words[0] & 4 else 0
    assert bool(tagged) == bool(hap)
    return hap, (None if p == phase.PS_NONE else p)


def test_the_hand_written_table(eng, tmp_path):
    refs, recs, sites, regions = TC.table_world()
    for block in (0xFF00, 1500):
        bam = str(tmp_path / ("table%d.bam" % block))
        bamio.write_bam(bam, refs, recs, block_size=block)
        status, n, answers = compare(eng, bam, regions, sites)
        assert status.tolist() == [0] * len(regions) and n == len(regions)
        for g, row in enumerate(TC.ROWS):
            locus = sites.rows(*regions[g][:3])
            assert one_read(answers[g]) == row[5] == phase.haplotag(row[1], row[2], row[3], locus), row[0]


def _ops_record(n_ops):
    """A CIGAR of n_ops operations - M at every even index and at the indices 63 and 127, I and D between them - and where
    every operation lies: (CIGAR, SEQ length, {index: (reference offset, query offset, length)} of the M operations)."""
    ops, where = [], {}
    r = q = 0
    for i in range(n_ops):
        if i % 2 == 0 or i in (63, 127):
            ops.append("3M")
            where[i] = (r, q, 3)
            r += 3
            q += 3
        elif i % 4 == 1:
            ops.append("1I")
            q += 1
        else:
            ops.append("2D")
            r += 2
    return "".join(ops), q, where


def test_tile_boundaries_of_operations_and_of_sites(eng, tmp_path):
    rng = np.random.default_rng(21)
    refs, recs, rows, regions, expect = [], [], [], [], []

    def add(cigar, seq, sites, pos=100, region=None):
        chrom = "k%d" % len(refs)
        refs.append((chrom, 200000))
        recs.append(("q%d" % len(recs), len(refs) - 1, pos - 1, cigar, seq))
        rows.extend((chrom, p, a1, a2, ps) for p, a1, a2, ps in sites)
        regions.append(region and (chrom,) + region or (chrom, pos, pos + 4, 20))
        expect.append(phase.haplotag(pos, cigar, seq, sorted(sites)))
        return expect[-1]

    other = {"A": "C", "C": "G", "G": "T", "T": "A"}
    # 65, 128 and 129 operations: one site in the operation at each tile's lane 0 and lane 63 (its last base), a region each,
    # then all of them together, on each operation's first base, voting the other way
    for n_ops in (65, 128, 129):
        cigar, l_seq, where = _ops_record(n_ops)
        seq = synth.random_dna(rng, l_seq)
        special = [i for i in (0, 63, 64, 127, 128) if i < n_ops]
        for i in special:
            r, q, n = where[i]
            assert add(cigar, seq, [(100 + r + n - 1, seq[q + n - 1], other[seq[q + n - 1]], 40 + i)]) == (1, 40 + i)
        every = [(100 + where[i][0], other[seq[where[i][1]]], seq[where[i][1]], 7) for i in special]
        assert add(cigar, seq, every) == (2, 7)
    # 63, 64 and 65 sites under one 400M record: the votes before the last site tie, the last one decides
    for ns in (63, 64, 65):
        seq = synth.random_dna(rng, 400)
        sites = []
        for i in range(ns):
            b = seq[3 * i]
            if i == ns - 1:
                sites.append((100 + 3 * i, other[b], b, 11))                             # haplotype 2
            elif i == 0 and (ns - 1) % 2:
                sites.append((100, other[b], other[other[b]], 11))                       # a third letter: no vote
            else:
                sites.append((100 + 3 * i, b, other[b], 11) if i % 2 else (100 + 3 * i, other[b], b, 11))
        assert add("400M", seq, sites) == (2, 11)
        assert phase.haplotag(100, "400M", seq, sites[:-1]) == (0, None)
    # a CG record of 70 001 operations, the deciding sites in its last operations
    cigar = "1M1I" * 35000 + "5000M"
    seq = "AC" * 35000 + "G" * 5000
    far = [(501 + 300, "C", "A", 3), (501 + 34999, "A", "C", 9), (501 + 39999, "G", "T", 9)]
    assert add(cigar, seq, far, pos=501, region=(1000, 3000, 500)) == (1, 9)
    assert phase.haplotag(501, cigar, seq, far[:1]) == (2, 3)
    # 64 phase sets (the last one, lane 63, has two votes), 65 (the host route), and a region without a site
    seq = synth.random_dna(rng, 400)
    many = [(100 + 3 * i, seq[3 * i], other[seq[3 * i]], 1000 + i) for i in range(63)] + \
           [(100 + 3 * i, other[seq[3 * i]], seq[3 * i], 1063) for i in (63, 64)]
    assert add("400M", seq, many) == (2, 1063)
    g65 = len(refs)
    assert add("400M", seq, many + [(100 + 3 * 65, seq[3 * 65], other[seq[3 * 65]], 999)]) == (2, 1063)
    assert add("400M", seq, []) == (0, None)
    sites = phase.Sites.from_rows(rows)
    bam = str(tmp_path / "tiles.bam")
    bamio.write_bam(bam, refs, recs, block_size=0xFF00)
    status, n, answers = compare(eng, bam, regions, sites)
    assert [g for g in range(len(regions)) if status[g]] == [g65] and status[g65] == 8 and n == len(regions) - 1
    for g in range(len(regions)):
        if g != g65:
            assert one_read(answers[g]) == expect[g], (g, regions[g])
    # the host route gives the region with 65 phase sets the same answer as the statement
    be = seqio.InProcessBam()
    got = be.chop(bam, *regions[g65], tagged=True, sites=sites)
    assert [tuple(r[3:]) for r in got] == [expect[g65]]


def test_a_full_slot_and_groups_above_the_cap(eng, tmp_path):
    rng = np.random.default_rng(23)
    contig = synth.random_dna(rng, 3000)
    site_pos = list(range(160, 690, 29))
    rows = [("c", p, contig[p - 1], {"A": "C", "C": "G", "G": "T", "T": "A"}[contig[p - 1]], 5 if p < 600 else 8) for p in site_pos]
    recs = []
    for i in range(256):
        pos = 100 + i % 50                                      # 1-based
        seq = bytearray(contig[pos - 1:pos - 1 + 600].encode())
        u = rng.random()
        for _c, p, ref, alt, _ps in rows:                       # a third of the reads each: haplotype 1 (REF), haplotype 2 (ALT), mixed
            if u < 0.33 or (u >= 0.66 and rng.random() < 0.5):
                continue
            seq[p - pos] = ord(alt)
        recs.append(("f%d" % i, 0, pos - 1, "600M", seq.decode()))
    bam = str(tmp_path / "full.bam")
    bamio.write_bam(bam, [("c", 3000)], recs, block_size=0xFF00)
    sites = phase.Sites.from_rows(rows)
    for keep in (20, 256):
        status, n, answers = compare(eng, bam, [("c", 300, 500, 100)], sites, max_keep=keep)
        tagged, p, words, _host = answers[0]
        sizes = [sum(1 for x in words if (x >> b) & 1) for b in range(3)]
        assert status.tolist() == [0] and tagged and p == 5
        assert sizes[0] == keep and sizes[1] >= 20 and sizes[2] >= 20 and (keep == 256 or sizes == [20, 20, 20])
    # one record more: beyond the 256 a region's slot holds - the host route's
    bamio.write_bam(bam, [("c", 3000)], recs + [("extra", 0, 99, "600M", contig[99:699])], block_size=0xFF00)
    status, _n, _a = compare(eng, bam, [("c", 300, 500, 100)], sites)
    assert status.tolist() == [4]


def _sorted(w):
    for c in w.reads:
        w.reads[c] = sorted(w.reads[c], key=lambda r: r.pos)
    return w


def _world_regions(w):
    """The region the deletion driver hands to chop_pacbio_read_by_pos, for every locus: all 30 reads of a locus start before it."""
    out = []
    for l in w.loci:
        f = min(500, len(l.ins_seq) if l.svtype == "INS" else l.end - l.start)
        out.append((l.chrom, l.start - f, l.start + f, f))
    return out + [("no_such_contig", 5, 900, 100)]


def test_the_truth_world_from_files(eng, tmp_path):
    w, snv = TC.truth_world()
    _sorted(w)
    sites = phase.Sites.from_rows((c, p, alt if gt == "1|0" else r, r if gt == "1|0" else alt, 1) for c, rows in snv.items() for p, r, alt, gt in rows)
    for block in (0xFF00, 1500):
        d = tmp_path / ("b%d" % block)
        d.mkdir()
        _fa, bam = synth.write_world_files(w, str(d), block_size=block)
        regions = _world_regions(w)
        status, n, answers = compare(eng, bam, regions, sites)
        assert status.tolist() == [0] * len(regions) and n >= 12 * 20
        for g, l in enumerate(w.loci):
            tagged, p, words, host = answers[g]
            assert tagged and p == 1 and sum(1 for x in words if x & 1) == 20
            assert all(hp in (1, 2) and ps == 1 for hp, ps in host)               # (every read got a haplotype, the host's view)


def test_a_damaged_block_sends_its_regions_to_the_host_route_and_no_other(eng, tmp_path):
    """One BGZF block fails its CRC in the inflate stage (the fixture of tests/test_gpu_bamdev.py).  The regions that hold the block
    come back with a status - they are the ones the host reader refuses as well, here as without the option - and every other
    region's answer is the host's on the undamaged file."""
    w, snv = TC.truth_world()
    _sorted(w)
    sites = phase.Sites.from_rows((c, p, alt if gt == "1|0" else r, r if gt == "1|0" else alt, 1) for c, rows in snv.items() for p, r, alt, gt in rows)
    _fa, good = synth.write_world_files(w, str(tmp_path), block_size=20000)
    raw = bytearray(open(good, "rb").read())
    bl = TB._blocks(bytes(raw))
    off, bsize, _xlen = bl[len(bl) // 2]
    raw[off + bsize - 8] ^= 0x40                                   # the block's CRC
    bad = str(tmp_path / "bad.bam")
    open(bad, "wb").write(bytes(raw))
    shutil.copy(good + ".bai", bad + ".bai")
    regions = _world_regions(w)
    status, n, answers = compare(eng, bad, regions, sites, host_bam=good)
    be = seqio.InProcessBam()
    refused = []
    for g, r in enumerate(regions):
        try:
            be.chop(bad, *r, tagged=True, sites=sites)
        except ValueError:
            refused.append(g)
    assert [g for g in range(len(regions)) if status[g]] == refused and 1 <= len(refused) <= 2 and all(status[g] == 5 for g in refused)
    assert len(answers) == len(w.loci) - len(refused) and n >= 20 * len(answers)


RUNS = [("device", {}, "hv"), ("host", {"VAPOR_BAM_DEVICE": "0"}, "hv"), ("drivers", {"VAPOR_FAST_PATH": "0"}, "hv"), ("truth", {}, "phased"),
        ("unphased", {}, None)]


def test_cli_tables_device_route_host_route_drivers_and_truth(tmp_path, monkeypatch):
    w, snv = TC.truth_world()
    _sorted(w)
    vcf = tmp_path / "snv.vcf"
    vcf.write_text(synth.snv_vcf_text(snv))
    bed = tmp_path / "in.bed"
    bed.write_text(synth.bed_text(w))
    files = {}
    for name, world in (("plain", w), ("tagged", _sorted(TC._tagged_copy(w)))):
        d = tmp_path / name
        d.mkdir()
        files[name] = synth.write_world_files(world, str(d), block_size=0xFF00)
    seen = []
    real = Engine.bam_chop_device

    def spy(self, *a, **k):
        got = real(self, *a, **k)
        seen.append((k.get("sites") is not None, bool(k.get("tagged")), got[4].tolist()))
        return got
    monkeypatch.setattr(Engine, "bam_chop_device", spy)
    monkeypatch.setenv("VAPOR_QC_SEED", "7")
    pipeline.set_engine(None)
    seqio.set_backend(seqio.InProcessBam())
    t = {}
    try:
        for name, env, kind in RUNS:
            for k in ("VAPOR_BAM_DEVICE", "VAPOR_FAST_PATH"):
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            fa, bam = files["tagged" if kind == "phased" else "plain"]
            o = tmp_path / (name + ".vapor")
            extra = ["--phase-vcf", str(vcf)] if kind == "hv" else ["--phased"] if kind == "phased" else []
            assert cli.main(["bed", "--sv-input", str(bed), "--reference", fa, "--pacbio-input", bam, "--output-path", str(tmp_path / "figs"),
                             "--output-file", str(o), "--no-figures"] + extra) == 0
            t[name] = o.read_bytes()
    finally:
        pipeline.set_engine(None)
        seqio.set_backend(None)
    # the device haplotagged every region of its run itself
    with_sites = [s for s in seen if s[0]]
    assert len(with_sites) == 1 and with_sites[0][1] and with_sites[0][2] == [0] * len(w.loci)
    assert t["device"] == t["host"] == t["drivers"] == t["truth"]
    rows = [ln.split("\t") for ln in t["device"].decode().splitlines()]
    assert [ln.split("\t") for ln in t["unphased"].decode().splitlines()] == [r[:10] for r in rows]
    assert len(rows) == 13 and all(r[10] == "1" for r in rows[1:])

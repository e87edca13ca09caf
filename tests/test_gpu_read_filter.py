"""The read filter on the device (vapor_bam_set_filter on the handle the four vapor_bam_chop_device* calls are made
with): every call with a filter against the host reader with the same filter AND against the same call without a filter on the
file written from the records that pass - kept reads, q0 / q1, miss_bp, member, phase set, tagged, status, and the bases behind every
address (the bit planes of a set made from the device addresses, vapor_seqset_create_mixed).  Small files on purpose: reads of
400-800 bases, windows of 300 bp, BGZF blocks of 2 KB, a region per way the kernel could go wrong."""
import numpy as np
import pytest

from vapor_amd import bamio, cli, phase, pipeline, seqio, synth
from vapor_amd import simple_function as SF
from vapor_amd.engine import Engine

pytestmark = pytest.mark.gpu

BLOCK = 2048
START, END, FLANK = 2000, 2300, 100
Q, F = 20, 0x904
KEPT_CAP, REG_NO_CIGAR, REG_KEPT_FULL, REG_NO_SEQ = 256, 3, 4, 7


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def passes(rec, q=Q, f=F):
    return not (rec[6] < q or (rec[7] & f))


def designed():
    """(refs, records, regions, sites): a contig per case, on each a window at 2000-2300 that a few passing records qualify for."""
    rng = np.random.default_rng(77)
    refs, recs, regions, sites = [], [], [], []
    bad = [(0, 0), (19, 16), (60, 4), (60, 0x100), (60, 0x800), (0, 0x904), (19, 0x900)]       # (MAPQ, FLAG) that (Q, F) filters
    good = [(60, 0), (20, 16), (255, 0), (60, 0x200), (60, 0x400), (59, 0x10)]                 # ... and that it does not

    def contig(name, n=6000):
        refs.append((name, n))
        ref = synth.random_dna(rng, n)
        for p in range(1710, 2000, 23):
            r = ref[p - 1]
            alt = "ACGT"[("ACGT".index(r) + 1 + p % 3) % 4]
            sites.append((name, p, r, alt, 5) if p % 2 else (name, p, alt, r, 5 if p % 3 else 6))
        return len(refs) - 1, ref

    def rec(tid, ref, name, pos0, mq, fl, n=None, cigar=None, seq=None):
        if cigar is None:
            seq, cigar = synth.mutate(rng, ref[pos0:pos0 + (n or int(rng.integers(400, 801)))])
        k = len(recs)
        recs.append((name, tid, pos0, cigar, seq, {"HP": 1 + k % 2, "PS": 7 if k % 4 else 9} if k % 5 else None, mq, fl))

    def kept_ones(tid, ref, tag, lo=1720, hi=1900, n=4):
        for i in range(n):
            rec(tid, ref, "%s_k%d" % (tag, i), int(rng.integers(lo, hi)), *good[(i + tid) % len(good)], n=int(rng.integers(700, 801)))

    # r0: a filtered record first in its span; r1: last in its span (the last record of the contig, still before the window start)
    t, ref = contig("r0")
    rec(t, ref, "first_f", 1500, *bad[0], n=800)
    kept_ones(t, ref, "r0", lo=1600)
    t, ref = contig("r1")
    kept_ones(t, ref, "r1")
    rec(t, ref, "last_f", 1995, *bad[1], n=800)
    # r2: three filtered records in a row between kept ones
    t, ref = contig("r2")
    rec(t, ref, "r2_a", 1700, *good[0], n=800)
    for i in range(3):
        rec(t, ref, "row_f%d" % i, 1750 + i, *bad[2 + i], n=780)
    rec(t, ref, "r2_b", 1800, *good[1], n=800)
    # r3: every record filtered
    t, ref = contig("r3")
    for i, (m, f) in enumerate(bad):
        rec(t, ref, "all_f%d" % i, 1700 + 20 * i, m, f, n=790)
    # r4: a filtered record whose header straddles two BGZF blocks (fillers in front of it take the padding that puts it there)
    t, ref = contig("r4")
    for i in range(14):
        rec(t, ref, "fill%02d" % i, 100 + i, *good[i % len(good)], n=400)
    rec(t, ref, "straddle_f", 1750, *bad[4], n=800)
    kept_ones(t, ref, "r4", lo=1760)
    # r5: filtered and kept records of 65 and of 129 operations (the walk goes 64 a step), the window start in the last operation
    t, ref = contig("r5")
    for k, (n_ops, (m, f)) in enumerate([(65, bad[0]), (65, good[0]), (129, bad[5]), (129, good[2])]):
        pairs = (n_ops - 1) // 2
        unit = [(4, "M"), (1, "I")] if n_ops == 65 else [(2, "M"), (1, "I")]
        ops = unit * pairs + [(700, "M")]
        q_len = sum(n for n, o in ops)
        rec(t, ref, "ops%d_%d" % (n_ops, k), 1800 + k, m, f, cigar="".join("%d%s" % o for o in ops), seq=synth.random_dna(rng, q_len))
    # r6: one filtered and one kept record whose 70 000 operations are in CG:B,I
    t, ref = contig("r6", 40000)
    for k, (m, f) in enumerate([bad[6], good[3]]):
        rec(t, ref, "cg%d" % k, 1900 + k, m, f, cigar="1M1I" * 35000, seq=synth.random_dna(rng, 70000))
    kept_ones(t, ref, "r6", n=2)
    # r7: a filtered unmapped mate without CIGAR on the window start; r8: a filtered secondary record without SEQ that the window
    # [START, START] would keep (the contig's other records end before it: a kept read of no bases is not what this is about)
    t, ref = contig("r7")
    rec(t, ref, "nocigar_f", START - 1, 0, 0x4 | 0x1, cigar="*", seq=synth.random_dna(rng, 500))
    kept_ones(t, ref, "r7")
    t, ref = contig("r8")
    rec(t, ref, "noseq_f", START - 1, 60, 0x100, cigar="100M", seq="")
    for i in range(3):
        rec(t, ref, "r8_before%d" % i, 1000 + i, *good[i], n=500)
    regions = [(name, START, END, FLANK) for name, _n in refs]
    regions[8] = ("r8", START, START, FLANK)
    return refs, recs, regions, sites


def _straddle_pad(path, refs, recs):
    """Writes the file so that the header of `straddle_f` crosses a block boundary: the fillers' names take the padding."""
    def where():
        b = bamio.BamFile(path)
        cur = b.bgzf.read_from(b.first_record)
        while True:
            at = cur.tell()
            hdr = cur.read(4)
            if len(hdr) < 4:
                return None
            r = cur.read(int.from_bytes(hdr, "little"))
            if r[32:32 + r[8] - 1] == b"straddle_f":
                return at & 0xFFFF
    bamio.write_bam(path, refs, recs, block_size=BLOCK)
    shift = (BLOCK - 20 - where()) % BLOCK
    out = []
    for r in recs:
        if r[0].startswith("fill") and shift:
            take = min(shift, 200)
            shift -= take
            r = (r[0] + "x" * take,) + r[1:]
        out.append(r)
    assert shift == 0
    bamio.write_bam(path, refs, out, block_size=BLOCK)
    u = where()
    assert u < BLOCK < u + 36, u                       # the 36 bytes the kernel loads first lie in two blocks
    return out


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_rf")
    refs, recs, regions, sites = designed()
    x = str(d / "x.bam")
    recs = _straddle_pad(x, refs, recs)
    p = str(d / "p.bam")
    bamio.write_bam(p, refs, [r for r in recs if passes(r)], block_size=BLOCK)
    assert sum(not passes(r) for r in recs) >= 18
    return x, p, regions, phase.Sites.from_rows(sites), recs


MODES = {"plain": {}, "right": {"right": True}, "tagged": {"groups": True}, "haplotag": {"groups": True}}


def device(eng, be, bam, regions, mode, sites, max_keep=20):
    """One device call; per region (status, [(q, miss, member, planes of the read's bases)]), and phase set / tagged per region."""
    kw = dict(MODES[mode])
    if mode == "haplotag":
        kw["sites"] = sites
    st = np.asarray([r[1] for r in regions], dtype=np.int64)
    en = np.asarray([r[2] for r in regions], dtype=np.int64)
    fl = np.asarray([r[3] for r in regions], dtype=np.int64)
    got = be.chop_many_device(eng, bam, [r[0] for r in regions], st, en, fl, max_keep, **kw)
    kf, addr, q, miss, status, batches = got[:6]
    member = got[6] if len(got) > 6 else np.zeros(len(addr), dtype=np.uint32)
    out = []
    try:
        lens = np.asarray([int(en[g] - st[g] - miss[t]) for g in range(len(regions)) for t in range(int(kf[g]), int(kf[g + 1]))], dtype=np.int64)
        planes = []
        if len(addr):
            ss = eng.seqset_raw(addr, lens, None, src_kind=np.full(len(addr), 2 if mode == "right" else 1, dtype=np.uint8), src_first=q)
            try:
                planes = [tuple(a.tobytes() for a in ss.planes(t)) for t in range(len(addr))]
            finally:
                ss.close()
        for g in range(len(regions)):
            out.append((int(status[g]), [(int(q[t]), int(miss[t]), int(member[t]), planes[t]) for t in range(int(kf[g]), int(kf[g + 1]))]))
    finally:
        for bt in batches:
            bt.close()
    extra = (got[7].tolist(), got[8].tolist()) if len(got) > 6 else None
    return out, extra


def host(eng, be, bam, regions, mode, sites, max_keep=20):
    """The host reader's answer in the same shape, without q (the host hands text): (status, [(miss, member, planes)])."""
    out = []
    texts = []
    if mode == "right":
        b = be._open(bam)
        for c, a, e, fl in regions:
            got = seqio.minimize_pacbio_read_list(b.chop_native(c, a, e, fl, right=True), max_keep)
            out.append([0, [(r[1], 0) for r in got]])
            texts += [r[0] for r in got]
        extra = None
    else:
        kw = dict(MODES[mode])
        if mode == "haplotag":
            kw["sites"] = sites
        import ctypes
        got = be.chop_many(bam, [r[0] for r in regions], [r[1] for r in regions], [r[2] for r in regions], [r[3] for r in regions], max_keep, **kw)
        kf, addr, q0, miss, status = got[:5]
        member = got[6] if len(got) > 6 else np.zeros(len(addr), dtype=np.uint32)
        for g, r in enumerate(regions):
            out.append([int(status[g]), [(int(miss[t]), int(member[t])) for t in range(int(kf[g]), int(kf[g + 1]))]])
            texts += [ctypes.string_at(int(addr[t]) + int(q0[t]), r[2] - r[1] - int(miss[t])).decode() for t in range(int(kf[g]), int(kf[g + 1]))]
        extra = (got[7].tolist(), got[8].tolist()) if len(got) > 6 else None
    planes = []
    if texts:
        ss = eng.seqset(texts)
        try:
            planes = [tuple(a.tobytes() for a in ss.planes(t)) for t in range(len(texts))]
        finally:
            ss.close()
    t = 0
    for g in range(len(out)):
        out[g] = (out[g][0], [(m, mem, planes[t + i]) for i, (m, mem) in enumerate(out[g][1])])
        t += len(out[g][1])
    return out, extra


@pytest.mark.parametrize("mode", list(MODES))
def test_device_with_a_filter_is_the_host_with_it_and_the_device_on_the_prefiltered_file(eng, files, mode):
    x, p, regions, sites, recs = files
    bx, bp, b0 = seqio.InProcessBam(), seqio.InProcessBam(), seqio.InProcessBam()
    bx.read_filter = (Q, F)
    dx, ex = device(eng, bx, x, regions, mode, sites)
    dp, ep = device(eng, bp, p, regions, mode, sites)
    assert dx == dp and ex == ep                                        # as if the filtered records were not in the file
    assert [s for s, _r in dx] == [0] * len(regions)                    # no filtered record leaves a status behind
    hx, eh = host(eng, bx, x, regions, mode, sites)
    assert [(s, [r[1:] for r in rd]) for s, rd in dx] == hx and ex == eh
    counts = [len(rd) for _s, rd in dx]
    assert counts[3] == 0 and all(counts[g] >= 2 for g in (0, 1, 2, 4, 5, 6, 7)), counts
    if mode in ("plain", "tagged"):
        assert counts[5] == 2 and counts[2] == 2                         # one record of 65 and one of 129 operations; the two around the row
    # without the filter the same file answers otherwise: the stoppers stop, the filtered records are kept
    d0, _e0 = device(eng, b0, x, regions, mode, sites)
    st0 = [s for s, _r in d0]
    if mode != "right":
        assert st0[7] == REG_NO_CIGAR and st0[8] == REG_NO_SEQ, st0
    assert len(d0[3][1]) == 7                                          # (every record of r3 qualifies: only the filter drops them)
    assert sum(len(rd) for _s, rd in d0) > sum(counts) or mode == "right"
    for be in (bx, bp, b0):
        for b in be._bam.values():
            b.close()


def test_kept_cap_counts_the_records_that_pass(eng, tmp_path):
    """300 short qualifying records in a region: with exactly 256 passing the slot holds them (status 0, 256 kept); with 257 the region
    is REG_KEPT_FULL, and the caller's host route answers it as the host reader answers the prefiltered file."""
    rng = np.random.default_rng(5)
    refs = [("k256", 4000), ("k257", 4000)]
    recs = []
    for tid, n_pass in ((0, 256), (1, 257)):
        ref = synth.random_dna(rng, 4000)
        drop = set(rng.permutation(300)[:300 - n_pass].tolist())
        for i in range(300):
            pos0 = 1850 + i % 140
            m, f = ((0, 0), (60, 0x100), (19, 0x800), (60, 4))[i % 4] if i in drop else ((60, 0), (20, 16), (255, 0x400))[i % 3]
            recs.append(("s%d_%d" % (tid, i), tid, pos0, "400M", ref[pos0:pos0 + 400], None, m, f))
    x, p = str(tmp_path / "cap.bam"), str(tmp_path / "cap_p.bam")
    bamio.write_bam(x, refs, recs, block_size=BLOCK)
    bamio.write_bam(p, refs, [r for r in recs if passes(r)], block_size=BLOCK)
    regions = [("k256", 2000, 2100, 50), ("k257", 2000, 2100, 50)]
    bx, bp = seqio.InProcessBam(), seqio.InProcessBam()
    bx.read_filter = (Q, F)
    dx, _ = device(eng, bx, x, regions, "plain", None, max_keep=KEPT_CAP)
    dp, _ = device(eng, bp, p, regions, "plain", None, max_keep=KEPT_CAP)
    assert dx == dp
    assert dx[0][0] == 0 and len(dx[0][1]) == 256 and dx[1] == (REG_KEPT_FULL, [])
    hx, _ = host(eng, bx, x, regions[:1], "plain", None, max_keep=KEPT_CAP)
    assert [(s, [r[1:] for r in rd]) for s, rd in dx[:1]] == hx
    # the region the device hands back: the per-locus host route, which filters identically
    seqio.set_backend(bx)
    try:
        final = seqio.chop_pacbio_read_by_pos(x, *regions[1])
    finally:
        seqio.set_backend(None)
    assert len(final) == 257 and final == bp.chop(p, *regions[1])
    for be in (bx, bp):
        for b in be._bam.values():
            b.close()


MARKS_904 = ("mapq0", "mapq_low", "unmapped", "secondary", "supplementary")


def _cli(tmp_path, name, mode, text, fa, bam, more):
    d = tmp_path / name
    d.mkdir()
    src = d / ("in." + mode)
    src.write_text(text)
    out = d / "out.vapor"
    seen = {}
    orig = SF.vcf_vapor_modify

    def keep_table(vcf_input, rec_new, *a, **k):
        seen["table"] = open(vcf_input + ".vapor").read()
        return orig(vcf_input, rec_new, *a, **k)
    SF.vcf_vapor_modify = keep_table
    try:
        assert cli.main([mode, "--sv-input", str(src), "--reference", fa, "--pacbio-input", bam, "--output-path", str(d / "figs"),
                         "--output-file", str(out), "--no-figures"] + list(more)) == 0
    finally:
        SF.vcf_vapor_modify = orig
    if mode == "vcf":
        return seen["table"], (d / "in.vcf.vapor").read_text()
    return out.read_text(), None


@pytest.mark.parametrize("case", ["bed", "vcf_bnd_both_ends", "bed_phase_vcf"])
def test_cli_from_files_decoy_world_with_the_filter_is_the_clean_world_without_it(tmp_path, case, monkeypatch):
    """12 loci from files, reads selected on the device: the table (and the annotated VCF) of the decoy world with
    --min-mapq 20 --exclude-flags 0x904 is, byte for byte, that of the clean world without the options."""
    monkeypatch.setenv("VAPOR_QC_SEED", "7")
    more, mode = [], "bed"
    if case == "vcf_bnd_both_ends":
        w = synth.make_bnd_world(41, forms=synth.BND_FORMS * 2, n_reads=8)
        for other in (synth.make_junction_world(42, n_reads=8),
                      synth.make_world(seed=43, n_loci=1, svtypes=("DEL",), span_range=(600, 900), read_len=3000, n_reads=8, alt_fraction=1.0)):
            w.contigs.update(other.contigs)
            w.reads.update(other.reads)
            w.loci += other.loci
        simple = synth.SynthWorld()
        simple.loci = [l for l in w.loci if l.svtype != "BND"]
        text, mode, more = synth.vcf_text(simple, header=False) + synth.bnd_vcf_text(w), "vcf", ["--bnd", "--both-ends"]
    else:
        w = synth.make_world(seed=44, n_loci=6, svtypes=("DEL", "INV", "TANDUP"), span_range=(300, 900), read_len=3000, n_reads=8, alt_fraction=1.0)
        null = synth.make_world(seed=45, n_loci=6, svtypes=("DEL", "INV", "INS"), span_range=(300, 900), read_len=3000, n_reads=8, alt_fraction=0.0,
                                chrom_prefix="n")
        w.contigs.update(null.contigs)
        w.reads.update(null.reads)
        w.loci += null.loci
        if case == "bed_phase_vcf":
            snv = synth.snv_world(w, 6)
            pv = tmp_path / "snv.vcf"
            pv.write_text(synth.snv_vcf_text(snv))
            more = ["--phase-vcf", str(pv)]
        text = synth.bed_text(w)
    assert len(w.loci) == 12
    d = synth.add_decoys(w, 23, marks=MARKS_904)
    for world in (w, d):
        for c in world.reads:
            world.reads[c] = sorted(world.reads[c], key=lambda r: r.pos)
    (tmp_path / "w").mkdir()
    (tmp_path / "d").mkdir()
    fa_w, bam_w = synth.write_world_files(w, str(tmp_path / "w"), block_size=BLOCK)
    fa_d, bam_d = synth.write_world_files(d, str(tmp_path / "d"), block_size=BLOCK)
    seqio.set_backend(seqio.InProcessBam())
    try:
        clean = _cli(tmp_path, "clean", mode, text, fa_w, bam_w, more)
        filtered = _cli(tmp_path, "filtered", mode, text, fa_d, bam_d, more + ["--min-mapq", "20", "--exclude-flags", "0x904"])
        assert pipeline.engine_slot(0).bam_last_stats()["regions"] > 0        # (the reads of that run were selected on the device)
    finally:
        seqio.set_backend(None)
    assert filtered == clean and clean[0].count("\n") >= 9 and clean[0].count("\tNA") < 6

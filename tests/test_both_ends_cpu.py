"""`--both-ends` on the host: the right-anchored chop in closed form against its definition - the existing chop
over the mirrored records - and the native helpers against that; every right-anchored view of a world W against the PRIMARY
view the existing code scores for the corresponding call in the reverse-complemented world M(W) (synth.mirror_world), every
extra left-anchored view against the record the existing code already scores in W; the seven columns; and every output
unchanged without the option.  Device work is answered by tests/fake_engine.py (oracle-backed, test only)."""
import numpy as np
import pytest

from fake_engine import FakeEngine
from vapor_amd import bothends, cli, drivers, finish, modes, pipeline, seqio, synth
from vapor_amd import simple_function as SF

F = 500
INS = ("", "ACGTTGCA", "GGA")


@pytest.fixture()
def fake(oracle):
    pipeline.set_engine(FakeEngine(oracle))
    yield
    pipeline.set_engine(None)
    seqio.set_backend(None)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the chop
# ------------------------------------------------------------------------------------------------------------------------------

def _random_records(seed, n, length, lower=True):
    rng = np.random.default_rng(seed)
    ref = synth.random_dna(rng, length)
    recs = []
    for i in range(n):
        a = int(rng.integers(0, length - 4000))
        read, cig = synth.mutate(rng, ref[a:a + int(rng.integers(300, 3500))])
        if i % 6 == 1:                                  # soft-clipped tail
            k = int(rng.integers(1, 700))
            cig, read = cig + "%dS" % k, read + synth.random_dna(rng, k)
        elif i % 6 == 2:                                # soft-clipped head
            k = int(rng.integers(1, 700))
            cig, read = "%dS" % k + cig, synth.random_dna(rng, k) + read
        elif i % 6 == 3:                                # IUPAC symbols, lower case, hard clips and padding around
            read = read[:5] + ("RYKMSWBDHVNryn=" if lower else "RYKMSWBDHVNRYN=") + read[20:]      # (a BAM file keeps no case)
            cig = "7H" + cig + "3P"
        recs.append(("q%d" % i, a + 1, cig, read))
    return ref, recs


def test_rc_of_a_read_is_position_reversal_and_nibble_bit_reversal():
    nt16 = "=ACMGRSVTWYHKDBN"
    for code, ch in enumerate(nt16):
        rev = int("{:04b}".format(code)[::-1], 2)
        assert seqio.rc_read(ch) == nt16[rev] and seqio.rc_read(ch.lower()) == nt16[rev].lower()
    assert seqio.rc_read("AC*gtX.N=") == "=N.Xac*GT"
    assert seqio.rc_read("AACG*x") == "x*CGTT"
    assert seqio.rc_read(seqio.rc_read("ACGTRYKMacgtn*=")) == "ACGTRYKMacgtn*="


def test_closed_form_chop_is_the_chop_of_the_mirrored_records():
    """Some thousands of records (synth.mutate, seed fixed) around one window, with a deletion straddling the window end, reads
    that end inside the window and tails that are soft clip only: reads, miss_bp and order are those of the definition; so are
    the native helpers' (vapor_chop_records_right over the records in memory)."""
    length = 12000
    ref, recs = _random_records(5, 4000, length)
    start, end, flank = 5000, 6000, 500
    recs += [("del_over_end", 4500, "1490M30D800M", "A" * 2290),        # reference 5990..6019 deleted: 5990..6000 miss, miss_bp 11
             ("ends_inside", 4500, "1200M", "G" * 1200),
             ("clip_only_tail", 4500, "1501M900S", "C" * 2401),          # last base = end: the walk ends in the clip
             ("clip_before_end", 4500, "1500M900S", "T" * 2400),         # last base end - 1: does not qualify
             ("ends_on_end", 4000, "2001M", "ACGT" * 500 + "A"),
             ("short_head", 5600, "600M", "ACGT" * 150),                 # too little SEQ before the window end
             ("big_del", 4000, "1801M400D900M", "ACG" * 900 + "A")]    # 5801..6200 deleted: miss_bp 200 <= flank / 2
    want = seqio._chop_records(seqio.mirror_records(recs, length), length + 1 - end, length + 1 - start, flank)
    got = seqio._chop_records(recs, start, end, flank, right=True)
    assert got == want and len(got) > 300
    names = [x[2] for x in got]
    for kept, miss in (("del_over_end", 11), ("clip_only_tail", 0), ("ends_on_end", 0), ("big_del", 200)):
        assert kept in names and got[names.index(kept)][1] == miss, kept
    for gone in ("ends_inside", "clip_before_end", "short_head"):
        assert gone not in names
    assert all(len(x[0]) == end - start - x[1] for x in got) and len({x[1] for x in got}) > 3
    # another window, another flank: L cancels (two different L give the same answer)
    for s2, e2, f2 in ((3000, 3400, 200), (7000, 8000, 100)):
        a = seqio._chop_records(seqio.mirror_records(recs, length), length + 1 - e2, length + 1 - s2, f2)
        b = seqio._chop_records(seqio.mirror_records(recs, length + 777), length + 778 - e2, length + 778 - s2, f2)
        assert a == b == seqio._chop_records(recs, s2, e2, f2, right=True) and len(a) > 20
    # the cap: smallest miss_bp first, record order inside one value
    many = seqio.minimize_pacbio_read_list(got)
    assert len(many) == 20 and [x[1] for x in many] == sorted(x[1] for x in many)
    # the native helpers on the same records
    w = synth.SynthWorld()
    w.contigs["c"] = ref
    w.reads["c"] = [synth.SamRecord(q, "c", p, c, s, sum(int(n) for n, o in seqio._CIGAR_RE.findall(c) if o in "M=D")) for q, p, c, s in recs]
    be = seqio.MemorySamtools(w)
    for s2, e2, f2 in ((start, end, flank), (3000, 3400, 200), (7000, 8000, 100)):
        py = seqio._chop_records([(r.qname, r.pos, r.cigar, r.seq) for r in w.overlapping("c", s2, e2)], s2, e2, f2, right=True)
        assert be.chop("x.bam", "c", s2, e2, f2, right=True) == py and len(py) > 20
    seqio.set_backend(be)
    try:
        assert seqio.chop_pacbio_read_by_pos("x.bam", "c", start, end, flank, right=True) == \
            [x for x in got if x[2] in {r.qname for r in w.overlapping("c", start, end)}]
        assert seqio.simple_del_chop_pacbio_read_simple_short("x.bam", ["c", 5500], 500, right=True) == many
    finally:
        seqio.set_backend(None)


def test_native_file_reader_and_many_regions_equal_python(tmp_path):
    """vapor_bam_chop_right (the host file route of InProcessBam) and vapor_chop_records_right_many on the same records."""
    import ctypes
    from vapor_amd import _lib
    length = 12000
    ref, recs = _random_records(6, 1500, length, lower=False)
    w = synth.SynthWorld()
    w.contigs["c"] = ref
    w.reads["c"] = sorted([synth.SamRecord(q, "c", p, c, s, sum(int(n) for n, o in seqio._CIGAR_RE.findall(c) if o in "M=D"))
                           for q, p, c, s in recs], key=lambda r: r.pos)
    fa, bam = synth.write_world_files(w, str(tmp_path), block_size=3000)
    ib = seqio.InProcessBam()
    regions = [(5000, 6000, 500), (3000, 3400, 200), (7000, 8000, 100), (1, 300, 100), (11000, 11900, 300)]
    lib = _lib.load()
    n = len(regions)
    mem = seqio.MemorySamtools(w)
    recs_c, arrs, ptr, _keep, _n = mem._arrays("c")
    for s2, e2, f2 in regions:
        py = seqio._chop_records([(r.qname, r.pos, r.cigar, r.seq) for r in w.overlapping("c", s2, e2)], s2, e2, f2, right=True)
        assert ib.chop(bam, "c", s2, e2, f2, right=True) == py
    assert sum(len(ib.chop(bam, "c", *r, right=True)) for r in regions) > 100
    st = np.asarray([r[0] for r in regions], dtype=np.int64)
    en = np.asarray([r[1] for r in regions], dtype=np.int64)
    fl = np.asarray([r[2] for r in regions], dtype=np.int64)
    n_rec = np.full(n, len(recs_c), dtype=np.int32)
    pp = np.asarray([ptr] * n, dtype=np.uint64).T.copy()
    keep = 20
    kf, idx = np.zeros(n + 1, dtype=np.int32), np.zeros(n * keep, dtype=np.int32)
    q1, miss, status = np.zeros(n * keep, dtype=np.int64), np.zeros(n * keep, dtype=np.int64), np.zeros(n, dtype=np.int32)
    assert lib.vapor_chop_records_right_many(n, n_rec.ctypes.data, pp[0].ctypes.data, pp[1].ctypes.data, pp[2].ctypes.data, pp[3].ctypes.data,
                                             st.ctypes.data, en.ctypes.data, fl.ctypes.data, keep, kf.ctypes.data, idx.ctypes.data,
                                             q1.ctypes.data, miss.ctypes.data, status.ctypes.data, None, None) == 0
    for g, (s2, e2, f2) in enumerate(regions):
        py = seqio.minimize_pacbio_read_list(seqio._chop_records(
            [(r.qname, r.pos, r.cigar, r.seq) for r in w.overlapping("c", s2, e2)], s2, e2, f2, right=True))
        got = []
        for t in range(int(kf[g]), int(kf[g + 1])):
            r = recs_c[int(idx[t])]
            stop = len(r.seq) - int(q1[t])
            got.append([seqio.rc_read(r.seq[stop - (e2 - s2 - int(miss[t])):stop]), int(miss[t]), r.qname])
        assert got == py and status[g] == 0, g
    ib._open(bam).close()


# ------------------------------------------------------------------------------------------------------------------------------
# 2. mirror equivalence
# ------------------------------------------------------------------------------------------------------------------------------

def _score_vcf(world, text, tmp_path, name, both_ends=False):
    """{key: (scores, views)} of `vapor vcf --bnd [--both-ends]` on a world in memory, through cli's own job list."""
    seqio.set_backend(seqio.MemorySamtools(world))
    vcf = tmp_path / (name + ".vcf")
    vcf.write_text(text)
    if both_ends:
        vl, _ = cli.vcf_list_readin(str(vcf), "ref.fa", True)
        jobs = cli.vcf_jobs(vl, 3, "x.bam", "ref.fa", str(tmp_path) + "/", "s", modes.BOTH_ENDS)
        scores = cli.score_jobs(jobs, 2048, None, modes.BOTH_ENDS)
    else:
        vl, _ = cli.vcf_list_readin(str(vcf), "ref.fa")
        jobs = cli.vcf_jobs(vl, 3, "x.bam", "ref.fa", str(tmp_path) + "/", "s")
        scores = cli.score_jobs(jobs, 2048, None)
    return {j.key: ([float(x) for x in s], j.extra) for j, s in zip(jobs, scores)}


def _kept(world, svtype, info, flank=F):
    """The number of reads every view of a locus keeps before the cap (primary view first)."""
    seqio.set_backend(seqio.MemorySamtools(world))
    out = []
    if svtype == "BND" and info[4] != "5to5":
        out.append(len(seqio.chop_pacbio_read_by_pos("x.bam", info[0], info[1] - flank, info[1] + flank, flank)))
    elif svtype != "BND":
        x = info[2] if svtype == "TANDUP" else info[1]
        out.append(len(seqio.chop_pacbio_read_by_pos("x.bam", info[0], x - flank, x + flank, flank)))
    for _name, _form, v, mirror in drivers.both_ends_views(svtype, info, flank):
        x = -v[1] if mirror else v[1]
        out.append(len(seqio.chop_pacbio_read_by_pos("x.bam", v[0], x - flank, x + flank, flank, right=mirror)))
    return out


def _bnd_text(records):
    return "\n".join("\t".join(r) for r in records) + "\n"


def _key(rec, both_ends=False):
    return cli.bnd_key(cli.bnd_view(rec[0], int(rec[1]), rec[4], both_ends))


BND_SEED = 11


def test_bnd_views_equal_the_primary_views_of_the_mirrored_world(fake, tmp_path):
    """All four forms, with and without inserted bases.  Every R view of `--bnd --both-ends` on W has exactly (== on float64,
    as sorted lists: M(W)'s records are sorted by their new POS) the per-read scores of the primary view of the corresponding
    record of mirror_world(W) under `--bnd` alone; the extra L view of a 3to3 record is the primary view of its mate written
    as the record, in W itself."""
    W = synth.make_bnd_world(BND_SEED, forms=synth.BND_FORMS * 3, n_reads=12, ins=INS)
    M = synth.mirror_world(W)
    rw, rm = synth.bnd_records(W), synth.bnd_records(M)
    got = _score_vcf(W, _bnd_text(rw), tmp_path, "w", both_ends=True)
    first_m = _score_vcf(M, _bnd_text(rm[0::2]), tmp_path, "m1")
    mate_m = _score_vcf(M, _bnd_text(rm[1::2]), tmp_path, "m2")
    mate_w = _score_vcf(W, _bnd_text(rw[1::2]), tmp_path, "w2")
    plain_w = _score_vcf(W, _bnd_text(rw), tmp_path, "w0")
    assert len(got) == len(W.loci) and len(plain_w) == len(W.loci) - 3          # (the 5to5 records: skipped without the option)
    passed = {}
    with_ins = set()
    for li, l in enumerate(W.loci):
        form = l.extra["form"]
        view = cli.bnd_view(rw[2 * li][0], int(rw[2 * li][1]), rw[2 * li][4], True)
        scores, views = got[_key(rw[2 * li], True)]
        kept = _kept(W, "BND", view)
        assert all(n <= 20 for n in kept), (form, kept)                          # the cap never chooses
        assert views is not None and len(views) == 2
        assert scores == (views[0] or [])
        with_ins.add((form, bool(l.ins_seq)))
        if form in ("3to5", "5to3"):
            assert scores == plain_w[_key(rw[2 * li])][0]                        # the primary view: as without the option
            exp = first_m[_key(rm[2 * li])][0]
            assert sorted(views[1] or []) == sorted(exp), (li, form)
            passed.setdefault(form, []).append(views[1] is not None and len(exp) > 0)
        elif form == "3to3":
            assert scores == plain_w[_key(rw[2 * li])][0]
            exp = mate_w[_key(rw[2 * li + 1])][0]
            assert (views[1] or []) == exp, (li, form)
            passed.setdefault(form, []).append(views[1] is not None and len(exp) > 0)
        else:
            exp_a, exp_b = first_m[_key(rm[2 * li])][0], mate_m[_key(rm[2 * li + 1])][0]
            assert sorted(views[0] or []) == sorted(exp_a) and sorted(views[1] or []) == sorted(exp_b), (li, form)
            passed.setdefault(form, []).append(views[0] is not None and views[1] is not None and len(exp_a) > 0 and len(exp_b) > 0)
    assert with_ins == {(f, b) for f in synth.BND_FORMS for b in (False, True)}
    assert all(any(v) for v in passed.values()) and set(passed) == set(synth.BND_FORMS), passed


JUNCTION_SEED = 12


def test_del_inv_tandup_views_equal_the_primary_views_of_the_mirrored_world(fake, tmp_path):
    """A DEL, an INV and a TANDUP of 12 kb read from both sides of their junctions (synth.make_junction_world): the R view(s) of
    each against the primary view of the mirrored call in M(W); the INV's L@e view against the `t]c:s]` breakend at c:e in W,
    its R@s view against that breakend of the mirrored call in M(W)."""
    W = synth.make_junction_world(JUNCTION_SEED)
    M = synth.mirror_world(W)
    fns = {"DEL": drivers.vapor_simple_del, "INV": drivers.vapor_simple_inv, "TANDUP": drivers.vapor_simple_tandup}

    def run(world, gen):
        seqio.set_backend(seqio.MemorySamtools(world))
        return pipeline.run_sync(gen)
    assert [l.svtype for l in W.loci] == ["DEL", "INV", "TANDUP"]
    for l, m in zip(W.loci, M.loci):
        info, minfo = [l.chrom, l.start, l.end], [m.chrom, m.start, m.end]
        n = len(W.contigs[l.chrom])
        assert minfo == [l.chrom, n + 1 - l.end, n + 1 - l.start]
        assert all(k <= 20 for k in _kept(W, l.svtype, info))
        got = run(W, drivers.vapor_both_ends(l.svtype, 3, 1, "x.bam", "ref.fa", info, "f.png"))
        plain = run(W, fns[l.svtype](3, 1, "x.bam", "ref.fa", info, "f.png"))
        assert list(got) == list(plain) == got.views[0] and len(plain) > 3
        primary_m = run(M, fns[l.svtype](3, 1, "x.bam", "ref.fa", minfo, "f.png"))
        if l.svtype == "INV":
            assert len(got.views) == 4 and all(v for v in got.views)
            assert got.views[1] == run(W, drivers.vapor_bnd(3, 1, "x.bam", "ref.fa", [l.chrom, l.end, l.chrom, l.start, "3to3", ""], "f.png"))
            assert sorted(got.views[2]) == sorted(primary_m)
            assert sorted(got.views[3]) == sorted(
                run(M, drivers.vapor_bnd(3, 1, "x.bam", "ref.fa", [m.chrom, m.end, m.chrom, m.start, "3to3", ""], "f.png")))
        else:
            assert len(got.views) == 2 and got.views[1] and sorted(got.views[1]) == sorted(primary_m)
    # mirror_world is an involution on what the chop reads
    MM = synth.mirror_world(M)
    assert MM.contigs == W.contigs and [(l.start, l.end) for l in MM.loci] == [(l.start, l.end) for l in W.loci]
    for c in W.reads:
        assert sorted((r.qname, r.pos, r.cigar, r.seq) for r in MM.reads[c]) == sorted((r.qname, r.pos, r.cigar, r.seq) for r in W.reads[c])


def test_short_loci_have_no_views_and_a_fall_through_has(fake):
    """A short DEL / INV / TANDUP that scores its short branch has no junction branch (views None); a short INV whose short
    branch finds too few reads falls through to the junction branch (SF:1917) and is then a junction locus."""
    w = synth.make_world(seed=31, n_loci=3, svtypes=("DEL", "INV", "TANDUP"), span_range=(600, 900), read_len=4000, n_reads=8)
    seqio.set_backend(seqio.MemorySamtools(w))
    for l in w.loci:
        got = pipeline.run_sync(drivers.vapor_both_ends(l.svtype, 3, 1, "x.bam", "ref.fa", [l.chrom, l.start, l.end], "f.png"))
        assert got.views is None and len(got) > 3
    inv = w.loci[1]
    got = pipeline.run_sync(drivers.vapor_both_ends("INV", 100, 1, "x.bam", "ref.fa", [inv.chrom, inv.start, inv.end], "f.png"))
    assert list(got) == [] and got.views == [None, None, None, None]


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the option and the columns
# ------------------------------------------------------------------------------------------------------------------------------

def _mixed_world():
    """Breakends of every form, a long DEL / INV / TANDUP read from both sides, and three short loci."""
    w = synth.make_bnd_world(BND_SEED, forms=synth.BND_FORMS, n_reads=12, ins=INS)
    for other in (synth.make_junction_world(JUNCTION_SEED),
                  synth.make_world(seed=31, n_loci=3, svtypes=("DEL", "INV", "TANDUP"), span_range=(600, 900), read_len=4000, n_reads=8)):
        w.contigs.update(other.contigs)
        w.reads.update(other.reads)
        w.loci += other.loci
    return w


def _mixed_vcf(w):
    simple = synth.SynthWorld()
    simple.loci = [l for l in w.loci if l.svtype != "BND"]
    plain = synth.vcf_text(simple, header=False).splitlines()
    brec = synth.bnd_vcf_text(w).splitlines()
    out = []
    for t in range(max(len(plain), len(brec))):
        out += plain[t:t + 1] + brec[t:t + 1]
    return "\n".join(out) + "\n"


def _main(tmp_path, name, mode, text, more=(), bnd=True):
    d = tmp_path / name
    d.mkdir()
    src = d / ("in." + mode)
    src.write_text(text)
    out = d / "out.vapor"
    args = [mode, "--sv-input", str(src), "--reference", "ref.fa", "--pacbio-input", "x.bam", "--output-path", str(d / "figs"),
            "--output-file", str(out), "--no-figures"] + (["--bnd"] if bnd and mode == "vcf" else []) + list(more)
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
    if mode == "vcf":
        return seen["table"], (d / "in.vcf.vapor").read_text()
    return out.read_text(), None


def test_columns_follow_the_views(fake, tmp_path):
    w = _mixed_world()
    seqio.set_backend(seqio.MemorySamtools(w))
    text = _mixed_vcf(w)
    table, final = _main(tmp_path, "on", "vcf", text, ["--both-ends"])
    rows = [r.split("\t") for r in table.splitlines()]
    assert rows[0][-7:] == list(bothends.COLUMNS) and all(len(r) == 13 for r in rows[1:])
    views = {k: v[1] for k, v in _score_vcf(w, text, tmp_path, "again", both_ends=True).items()}
    seqio.set_backend(seqio.MemorySamtools(w))
    assert len(rows) - 1 == len(views) == 4 + 2 + 2                              # (vcf mode buckets TANDUP and never scores it)
    n_junction = 0
    for r in rows[1:]:
        v = views[r[0]]
        if v is None:
            assert r[6:] == ["."] * 7 and (r[0].endswith(":DEL") or r[0].endswith(":INV"))
            continue
        n_junction += 1
        scored = [x for x in v if x is not None]
        cat = [s for x in scored for s in x]
        assert r[6] == str(len(scored)) and r[7:12] == [str(x) for x in finish.row_tail(cat)]
        tail = SF.format_output_row(finish.result_organize_ins(["k", cat])).split("\t")      # the reference-named routines
        assert r[7:12] == tail[1:] or not cat
        assert r[12] == ",".join("." if x is None else str(finish.row_tail(x)[0]) for x in v)
        assert r[1:6] == [str(x) for x in finish.row_tail(v[0] or [])]           # the row's own five: the primary view's
    assert n_junction == 4 + 2
    # the gate: with --PB-supp 9 a view of fewer than ten reads is '.', and BE_N counts the rest
    table9, _ = _main(tmp_path, "on9", "vcf", text, ["--both-ends", "--PB-supp", "9"])
    rows9 = [r.split("\t") for r in table9.splitlines()[1:]]
    gated = [r for r in rows9 if r[12] != "." and "." in r[12].split(",")]
    assert gated and all(int(r[6]) == sum(1 for x in r[12].split(",") if x != ".") for r in rows9 if r[6] != ".")
    # the annotated VCF: the seven as INFO keys, '.' keys left out, both mates of a pair alike, ##INFO lines only with a header
    recs = [x.split("\t") for x in final.splitlines() if x and not x.startswith("#")]
    by_id = {x[2]: x for x in recs}
    n_mates = 0
    for x in recs:
        if "SVTYPE=BND" in x[7]:
            assert ";VaPoR_BE_N=" in x[7] and ";VaPoR_BE_SQS=" in x[7] and ";VaPoR_BE_Rec=" in x[7]
            mate = by_id[x[7].split("MATEID=")[1].split(";")[0]]
            assert x[7].split(";VaPor_GS=")[1] == mate[7].split(";VaPor_GS=")[1]
            n_mates += 1
        elif "END=" in x[7] and int(x[7].split("END=")[1].split(";")[0]) - int(x[1]) < 10000:
            assert "VaPoR_BE_" not in x[7] and ";VaPor_GS=" in x[7]
    assert n_mates == 8
    head = "##fileformat=VCFv4.2\n##INFO=<ID=SVTYPE,Number=1,Type=String,Description=\"t\">\n##source=x\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n"
    _t, final_h = _main(tmp_path, "hdr", "vcf", head + text, ["--both-ends"])
    assert all("##INFO=<ID=%s," % c in final_h for c in bothends.COLUMNS)
    # bed: TANDUP too
    bed = synth.bed_text(w)
    tb, _ = _main(tmp_path, "bed_on", "bed", bed, ["--both-ends"])
    rb = [r.split("\t") for r in tb.splitlines()]
    assert rb[0][-7:] == list(bothends.COLUMNS) and len(rb) == 1 + 6
    long_rows = [r for r in rb[1:] if int(r[2]) - int(r[1]) >= 10000]
    assert [r[3] for r in long_rows] == ["DEL", "INV", "TANDUP"] and [r[10] for r in long_rows] == ["2", "4", "2"]
    assert all(r[10:] == ["."] * 7 for r in rb[1:] if r not in long_rows)


def test_pack_and_unpack_and_job_cost():
    for v in (None, [None], [[0.5, -1.25], None, []], [[1.0]]):
        assert bothends.unpack(bothends.pack(v)) == v
    assert bothends.columns_many([None]) == [["."] * 7]
    assert bothends.columns_many([[None, None]]) == [["0", "NA", "NA", "NA", "NA", "NA", ".,."]]
    assert cli.job_cost("DEL", 20000, views=2) > cli.job_cost("DEL", 20000) == cli.job_cost("DEL", 20000, views=1)
    assert cli.job_cost("INV", 20000, views=4) > cli.job_cost("INV", 20000, views=2)


@pytest.mark.parametrize("other", [["--refine", "50"], ["--phased"]])
def test_the_option_is_refused_with_refine_and_with_phased(other, tmp_path, capsys):
    src = tmp_path / "in.bed"
    src.write_text("c\t1\t2\tid\tDEL\n")
    with pytest.raises(SystemExit):
        cli.main(["bed", "--sv-input", str(src), "--reference", "r", "--pacbio-input", "b", "--output-path", str(tmp_path), "--output-file",
                  str(tmp_path / "o"), "--no-figures", "--both-ends"] + other)
    assert "--both-ends and " + other[0] + " cannot be combined" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["svelter", "--sv-input", str(src), "--reference", "r", "--pacbio-input", "b", "--output-path", str(tmp_path),
                  "--output-file", str(tmp_path / "o"), "--both-ends"])


# ------------------------------------------------------------------------------------------------------------------------------
# 4. unchanged without the option
# ------------------------------------------------------------------------------------------------------------------------------

def test_outputs_unchanged_without_the_option_and_old_columns_unchanged_with_it(fake, tmp_path, capsys):
    w = _mixed_world()
    seqio.set_backend(seqio.MemorySamtools(w))
    text, bed = _mixed_vcf(w), synth.bed_text(w)
    capsys.readouterr()
    t0, v0 = _main(tmp_path, "off1", "vcf", text)
    err0 = [x for x in capsys.readouterr().err.splitlines() if "skipped" in x]
    t1, v1 = _main(tmp_path, "off2", "vcf", text)
    capsys.readouterr()
    assert (t0, v0) == (t1, v1) and "VaPoR_BE" not in t0 + v0
    rec5 = [r for r in synth.bnd_records(w) if r[4].startswith("[")]
    assert len(err0) == 2 and all("5to5 junction: its reads are clipped on the left, which the read model (SF:339-354) does not take" in x
                                  for x in err0)
    assert err0[0] == "vapor vcf --bnd: record %s:%s %s skipped: %s" % (rec5[0][0], rec5[0][1], rec5[0][4], cli.bnd_view(rec5[0][0], int(rec5[0][1]), rec5[0][4]))
    t2, v2 = _main(tmp_path, "on", "vcf", text, ["--both-ends"])
    assert not [x for x in capsys.readouterr().err.splitlines() if "skipped" in x]
    old = {r.split("\t")[0]: r.split("\t") for r in t0.splitlines()}
    new = {r.split("\t")[0]: r.split("\t") for r in t2.splitlines()}
    assert set(new) - set(old) == {k for k in new if ":5to5:BND" in k} and len(set(new) - set(old)) == 1 and set(old) <= set(new)
    assert [r.split("\t")[0] for r in t2.splitlines() if r.split("\t")[0] in old] == [r.split("\t")[0] for r in t0.splitlines()]
    for k, r in old.items():
        assert new[k][:len(r)] == r, k
    def no_be(line):
        f = line.split("\t")
        if len(f) > 7:
            f[7] = ";".join(x for x in f[7].split(";") if not x.startswith("VaPoR_BE_"))
        return "\t".join(f)
    # (the annotated VCF holds the scored records: the 5to5 pair is there with the option only)
    on = [x for x in v2.splitlines() if "\t[" not in x]
    assert v0.splitlines() == [no_be(x) for x in on] and len(on) == len(v2.splitlines()) - 2
    assert all(";VaPor_GS=" in x and ";VaPoR_BE_N=" in x for x in v2.splitlines() if "\t[" in x)
    b0, _ = _main(tmp_path, "bed_off1", "bed", bed)
    b1, _ = _main(tmp_path, "bed_off2", "bed", bed)
    b2, _ = _main(tmp_path, "bed_on", "bed", bed, ["--both-ends"])
    assert b0 == b1 and [r.split("\t")[:10] for r in b2.splitlines()] == [r.split("\t") for r in b0.splitlines()]
    # bnd_view's default answers are what they were
    assert "5to5" in cli.bnd_view("c1", 1000, "[c5:1200[A") and isinstance(cli.bnd_view("c1", 1000, "[c5:1200[A"), str)
    assert cli.bnd_view("c1", 1000, "[c5:1200[GA", True) == ["c1", 1000, "c5", 1200, "5to5", "G"]


def test_exports_and_header():
    import os
    from conftest import ROOT
    from vapor_amd import _lib as L
    new = ("vapor_chop_records_right", "vapor_chop_records_right_many", "vapor_bam_chop_right", "vapor_bam_chop_device_right")
    h = open(os.path.join(ROOT, "include", "vapor_hip.h")).read()
    for name in new:
        assert name in L.EXPORTS and name in L.OPTIONAL_EXPORTS and name + "(" in h
    assert L.ABI_VERSION == 3 and "src_kind[i] = 2" in h

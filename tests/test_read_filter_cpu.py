"""`--min-mapq` / `--exclude-flags` on the host.  The reference has no filter, so the statement tested against is
the definition: reading file X with (Q, F) equals reading, without a filter, the file written from exactly the records of X that
pass - per route (the Python statement, the four native readers, MemorySamtools, SAM text), at the edges of the rule, where a
record that stops a region today is filtered, for the majority phase set of `--phased`, and end to end through cli.main on worlds
with planted decoys (synth.add_decoys).  Device work is answered by tests/fake_engine.py (oracle-backed, test only)."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

from fake_engine import FakeEngine
from vapor_amd import _lib as L
from vapor_amd import bamio, cli, phase, pipeline, seqio, synth
from vapor_amd import simple_function as SF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPQS = (0, 1, 19, 20, 59, 60, 255)
FLAGS = (0, 16, 4, 0x100, 0x200, 0x400, 0x800, 0x904)
FILTERS = ((20, 0x904), (1, 0), (0, 4), (60, 16), (255, 0x200), (21, 0xFFFF))
CONTIG = 24000
BLOCK = 700                       # bytes of BAM stream per BGZF block: every record crosses blocks


@pytest.fixture()
def fake(oracle):
    pipeline.set_engine(FakeEngine(oracle))
    yield
    pipeline.set_engine(None)
    seqio.set_backend(None)


def passes(mapq, flag, q, f):
    return not (mapq < q or (flag & f))


# ------------------------------------------------------------------------------------------------------------------------------
# the files: every MAPQ x FLAG of the two lists, reads that start before, inside and behind the windows
# ------------------------------------------------------------------------------------------------------------------------------
def file_records(seed=11):
    """(refs, records for bamio.write_bam, phased sites): 2 x 56 records on contig c - all MAPQ x FLAG pairs twice - with HP / PS
    tags on two of three, soft clips on some, and a second contig d with a few records that no window of c may see."""
    rng = np.random.default_rng(seed)
    ref = synth.random_dna(rng, CONTIG)
    recs = []
    combos = [(m, f) for m in MAPQS for f in FLAGS]
    for i, (m, f) in enumerate(combos + combos):
        a = int(rng.integers(0, 9000)) if i % 4 else int(rng.integers(9000, 12000))
        read, cig = synth.mutate(rng, ref[a:a + int(rng.integers(3000, 9000))])
        if i % 7 == 3:
            cig, read = "9S" + cig, "ACGTTGCAA" + read
        tags = {"HP": 1 + (i // 3) % 2, "PS": 7 if i % 5 else 9} if i % 3 else None
        recs.append(("q%d" % i, 0, a, cig, read, tags, m, f))
    for i in range(4):
        recs.append(("other%d" % i, 1, 100 * i, "50M", "ACGTA" * 10, None, 0 if i % 2 else 60, 0))
    sites = []
    for p in range(8000, 12001, 37):
        r = ref[p - 1]
        alt = "ACGT"[("ACGT".index(r) + 1 + p % 3) % 4]
        sites.append(("c", p, r, alt, 5) if p % 2 else ("c", p, alt, r, 5 if p % 3 else 6))
    return [("c", CONTIG), ("d", 5000)], recs, phase.Sites.from_rows(sites)


WINDOWS = [(9500, 10000, 500), (10100, 10900, 200), (11990, 12400, 1000), (12100, 12101, 2), (8000, 8300, 10)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("rf")
    refs, recs, sites = file_records()
    x = str(d / "x.bam")
    bamio.write_bam(x, refs, recs, block_size=BLOCK)
    pre = {}
    for q, f in FILTERS:
        p = str(d / ("p_%d_%d.bam" % (q, f)))
        bamio.write_bam(p, refs, [r for r in recs if passes(r[6], r[7], q, f)], block_size=BLOCK)
        pre[(q, f)] = p
    return x, pre, sites, recs, refs


def world_of(refs, recs):
    w = synth.SynthWorld()
    for name, n in refs:
        w.contigs[name] = "A" * n
        w.reads[name] = []
    for qname, tid, pos0, cig, seq, tags, m, f in sorted(recs, key=lambda r: (r[1], r[2])):
        span = sum(int(k) for k, op in seqio._CIGAR_RE.findall(cig) if op in "MDN=X")
        w.reads[refs[tid][0]].append(synth.SamRecord(qname, refs[tid][0], pos0 + 1, cig, seq, max(span, 1), tags, f, m))
    return w


# ------------------------------------------------------------------------------------------------------------------------------
# parser
# ------------------------------------------------------------------------------------------------------------------------------
BASE = ["--reference", "r", "--pacbio-input", "b", "--no-figures"]


def test_parser_takes_decimal_and_hex_and_refuses_the_rest(capsys):
    p = cli.build_parser()
    core = ["--sv-input", "x", "--output-path", "o", "--output-file", "f"] + BASE
    a = p.parse_args(core)
    assert (a.min_mapq, a.exclude_flags) == (0, 0)
    a = p.parse_args(core + ["--min-mapq", "20", "--exclude-flags", "0x904"])
    assert (a.min_mapq, a.exclude_flags) == (20, 0x904)
    a = p.parse_args(core + ["--min-mapq", "0xff", "--exclude-flags", "65535"])
    assert (a.min_mapq, a.exclude_flags) == (255, 65535)
    for opt, bad in (("--min-mapq", "-1"), ("--min-mapq", "256"), ("--exclude-flags", "65536"), ("--exclude-flags", "-1"),
                     ("--min-mapq", "twenty"), ("--exclude-flags", "0x"), ("--min-mapq", "2.5"), ("--exclude-flags", "")):
        with pytest.raises(SystemExit):
            p.parse_args(core + [opt, bad])
        assert opt in capsys.readouterr().err


@pytest.mark.parametrize("cmd", ["bed", "vcf", "svelter", "ins"])
def test_all_four_subcommands_take_the_options_and_set_the_backend_once(cmd, tmp_path, monkeypatch, capsys):
    """The run sees (Q, F) on the backend the reads are taken through; without the options it sees (0, 0); after the run the
    backend is as it was; a value out of range is a parser error on every sub-command."""
    from vapor_amd import melt
    src = tmp_path / ("in." + ("vcf" if cmd == "vcf" else "bed"))
    src.write_text("")
    be = seqio.MemorySamtools(synth.SynthWorld())
    seqio.set_backend(be)
    seen = []
    monkeypatch.setattr(cli, "score_jobs", lambda jobs, *a, **k: seen.append(seqio.get_backend().read_filter) or [])
    monkeypatch.setattr(melt, "run", lambda *a, **k: seen.append(seqio.get_backend().read_filter))
    monkeypatch.setattr(SF, "vcf_vapor_modify", lambda *a, **k: None)
    args = [cmd, "--sv-input", str(src), "--output-path", str(tmp_path / "figs"), "--output-file", str(tmp_path / "out")] + BASE
    try:
        assert cli.main(args) == 0
        assert cli.main(args + ["--min-mapq", "20", "--exclude-flags", "0x904"]) == 0
        assert cli.main(args + ["--min-mapq", "0", "--exclude-flags", "0"]) == 0
        assert seen == [(0, 0), (20, 0x904), (0, 0)] and be.read_filter == (0, 0)
        with pytest.raises(SystemExit):
            cli.main(args + ["--min-mapq", "256"])
        assert "--min-mapq" in capsys.readouterr().err
    finally:
        seqio.set_backend(None)


def test_workflow_forwards_the_options(tmp_path, monkeypatch):
    from vapor_amd import workflow
    got = []

    def fake_main(argv):
        got.append(list(argv))
        open(argv[argv.index("--output-file") + 1], "w").write("CHR\tPOS\tEND\n")
        return 0
    monkeypatch.setattr(cli, "main", fake_main)
    src = tmp_path / "in.bed"
    src.write_text("")
    argv = ["bed", "--sv-input", str(src), "--output-path", str(tmp_path / "f"), "--output-file", str(tmp_path / "o")] + BASE + \
           ["--min-mapq", "20", "--exclude-flags", "0x704"]
    assert workflow.main(["--gpus", "1", "--no-index"] + argv) == 0
    assert got and got[0][-4:] == ["--min-mapq", "20", "--exclude-flags", "0x704"]
    # what arrives is what the command line's own parser reads
    a = cli.build_parser().parse_args(got[0][1:])
    assert (a.min_mapq, a.exclude_flags) == (20, 0x704)


# ------------------------------------------------------------------------------------------------------------------------------
# the rule's edges, one record each
# ------------------------------------------------------------------------------------------------------------------------------
EDGES = [  # (MAPQ, FLAG, Q, F, kept)
    (20, 0, 20, 0, True), (19, 0, 20, 0, False), (255, 0, 255, 0, True), (254, 0, 255, 0, False), (0, 0, 0, 0, True),
    (60, 0x10, 60, 0x900, True), (60, 0x910, 60, 0x900, False), (60, 0x100, 0, 0x900, False), (60, 0x800, 0, 0x900, False),
    (0, 0xFFFF, 0, 0, True), (60, 0x8000, 0, 0x8000, False), (60, 0x7FFF, 0, 0x8000, True),
]


def test_edges_of_the_rule_on_one_record_each(tmp_path):
    rng = np.random.default_rng(3)
    ref = synth.random_dna(rng, 4000)
    read, cig = synth.mutate(rng, ref[100:3000])
    be = seqio.InProcessBam()
    for t, (m, f, q, flt, kept) in enumerate(EDGES):
        assert bamio.record_passes(m, f, q, flt) == kept
        path = str(tmp_path / ("e%d.bam" % t))
        bamio.write_bam(path, [("c", 4000)], [("one", 0, 100, cig, read, {"HP": 1, "PS": 3}, m, f)], block_size=BLOCK)
        plain = be.chop(path, "c", 600, 1200, 100)
        assert len(plain) == 1
        be.read_filter = (q, flt)
        want = plain if kept else []
        assert be.chop(path, "c", 600, 1200, 100) == want and be.chop_python(path, "c", 600, 1200, 100) == want, (m, f, q, flt)
        assert [r[:3] for r in be.chop(path, "c", 600, 1200, 100, tagged=True)] == want
        assert len(be.chop(path, "c", 600, 1200, 100, right=True)) == len(want)
        w = world_of([("c", 4000)], [("one", 0, 100, cig, read, None, m, f)])
        mem = seqio.MemorySamtools(w)
        mem.read_filter = (q, flt)
        assert mem.chop("x", "c", 600, 1200, 100) == want
        assert np.diff(mem.chop_many("x", ["c"], [600], [1200], [100])[0]).tolist() == [len(want)]
        be.read_filter = (0, 0)
    # the C entry refuses what is out of range and takes the limits
    lib = L.load()
    tl = be._open(path)._take_handle(lib)
    for q, flt, ok in ((0, 0, True), (255, 65535, True), (-1, 0, False), (256, 0, False), (0, 65536, False), (0, 0xFFFFFFFF, False)):
        assert (lib.vapor_bam_set_filter(tl["native"], q, flt) == 0) == ok, (q, flt)
    assert lib.vapor_bam_set_filter(None, 0, 0) == L.E_ARG
    lib.vapor_bam_set_filter(tl["native"], 0, 0)
    for bad in ((-1, 0), (256, 0), (0, 65536)):
        with pytest.raises(ValueError):
            bamio.check_filter(*bad)


# ------------------------------------------------------------------------------------------------------------------------------
# as if absent, per route
# ------------------------------------------------------------------------------------------------------------------------------
def _many(be, src, regions, **kw):
    got = be.chop_many(src, ["c"] * len(regions), [r[0] for r in regions], [r[1] for r in regions], [r[2] for r in regions], **kw)
    kf, addr, q0, miss, status = got[:5]
    reads = [[ctypes.string_at(int(addr[t]) + int(q0[t]), r[1] - r[0] - int(miss[t])).decode() for t in range(int(kf[g]), int(kf[g + 1]))]
             for g, r in enumerate(regions)]
    rest = [np.asarray(a).tolist() for a in got[6:]]
    return np.diff(kf).tolist(), reads, miss.tolist(), status.tolist(), rest


@pytest.mark.parametrize("flt", FILTERS)
def test_file_routes_read_x_filtered_as_the_prefiltered_file(files, flt, monkeypatch):
    """chop_python, vapor_bam_chop, _tagged, _haplotag, _right and chop_many: entry by entry read, miss_bp, qname, hap, ps."""
    x, pre, sites, recs, _refs = files
    monkeypatch.delenv("VAPOR_BAM_NATIVE", raising=False)
    bx, bp = seqio.InProcessBam(), seqio.InProcessBam()
    bx.read_filter = flt
    n_seen = 0
    for (a, b, fl) in WINDOWS:
        for kw in ({}, {"tagged": True}, {"tagged": True, "sites": sites}):
            want = bp.chop_python(pre[flt], "c", a, b, fl, **kw)
            assert bx.chop_python(x, "c", a, b, fl, **kw) == want
            assert bx.chop(x, "c", a, b, fl, **kw) == want and bp.chop(pre[flt], "c", a, b, fl, **kw) == want
            n_seen += len(want)
        want = bp.chop(pre[flt], "c", a, b, fl, right=True)
        assert bx.chop(x, "c", a, b, fl, right=True) == want
        monkeypatch.setenv("VAPOR_BAM_NATIVE", "0")
        assert bx.chop(x, "c", a, b, fl, right=True) == want and bx.chop(x, "c", a, b, fl) == bp.chop(pre[flt], "c", a, b, fl)
        monkeypatch.delenv("VAPOR_BAM_NATIVE")
        assert bx.records(x, "c", a, b) == bp.records(pre[flt], "c", a, b)
        assert bx.view_lines(x, "c:%d-%d" % (a, b)) == bp.view_lines(pre[flt], "c:%d-%d" % (a, b))
    for kw in ({}, {"groups": True}, {"groups": True, "sites": sites}, {"max_keep": 3}):
        assert _many(bx, x, WINDOWS, **kw) == _many(bp, pre[flt], WINDOWS, **kw)
    # the filter decides something here: the unfiltered reading of X differs (unless every record of X passes)
    plain = seqio.InProcessBam()
    assert any(plain.chop(x, "c", a, b, fl) != bx.chop(x, "c", a, b, fl) for a, b, fl in WINDOWS)
    assert n_seen > 0 or flt == (21, 0xFFFF)


@pytest.mark.parametrize("flt", FILTERS)
def test_memory_and_text_routes_read_the_world_filtered_as_the_prefiltered_world(files, flt, monkeypatch):
    _x, _pre, sites, recs, refs = files
    wx, wp = world_of(refs, recs), world_of(refs, [r for r in recs if passes(r[6], r[7], *flt)])
    mx, mp = seqio.MemorySamtools(wx), seqio.MemorySamtools(wp)
    mx.read_filter = flt

    class Text:                      # a backend that answers in SAM text alone, as the samtools binary's does
        read_filter = flt
        view_lines = seqio.MemorySamtools(wx).view_lines

    class TextPre:
        view_lines = mp.view_lines
    for (a, b, fl) in WINDOWS:
        for kw in ({}, {"tagged": True}, {"tagged": True, "sites": sites}, {"right": True}):
            want = mp.chop("x", "c", a, b, fl, **kw)
            assert mx.chop("x", "c", a, b, fl, **kw) == want
            monkeypatch.setenv("VAPOR_MEMORY_CHOP", "records")
            assert mx.chop("x", "c", a, b, fl, **kw) == want
            monkeypatch.delenv("VAPOR_MEMORY_CHOP")
            seqio.set_backend(Text())
            got = seqio.chop_pacbio_read_by_pos("x", "c", a, b, fl, **kw)
            seqio.set_backend(TextPre())
            assert got == seqio.chop_pacbio_read_by_pos("x", "c", a, b, fl, **kw) == want
            seqio.set_backend(None)
        assert mx.records("x", "c", a, b) == mp.records("x", "c", a, b)
        assert mx.view_lines("x", "c:%d-%d" % (a, b)) == mp.view_lines("x", "c:%d-%d" % (a, b))
    for kw in ({}, {"groups": True}, {"groups": True, "sites": sites}, {"max_keep": 3}):
        assert _many(mx, "x", WINDOWS, **kw) == _many(mp, "x", WINDOWS, **kw)
    # a filter set later, or changed, is the one applied (the per-contig arrays are made from the records that pass)
    mx.read_filter = (0, 0)
    full = seqio.MemorySamtools(wx)
    assert _many(mx, "x", WINDOWS) == _many(full, "x", WINDOWS)
    mx.read_filter = flt
    assert _many(mx, "x", WINDOWS) == _many(mp, "x", WINDOWS)
    # the files and the worlds hold the same records: the two families agree with each other as well
    assert [r[:3] for r in mx.chop("x", "c", *WINDOWS[0])] == [r[:3] for r in seqio.InProcessBam().chop(_pre[flt], "c", *WINDOWS[0])]


def test_a_library_without_the_entry_sends_a_filtered_run_through_the_python_statement(files, monkeypatch):
    x, pre, _sites, _recs, _refs = files
    flt = FILTERS[0]
    real = L.load()

    class Without:
        def __getattr__(self, name):
            if name == "vapor_bam_set_filter":
                raise AttributeError(name)
            return getattr(real, name)
    bp = seqio.InProcessBam()
    want = [bp.chop(pre[flt], "c", a, b, fl) for a, b, fl in WINDOWS]
    want_r = [bp.chop(pre[flt], "c", a, b, fl, right=True) for a, b, fl in WINDOWS]
    assert "vapor_bam_set_filter" in L.EXPORTS and "vapor_bam_set_filter" in L.OPTIONAL_EXPORTS and L.ABI_VERSION == 3
    monkeypatch.setattr(L, "_lib", Without())
    be = seqio.InProcessBam()
    assert be.chop(x, "c", *WINDOWS[0]) == seqio.InProcessBam().chop(x, "c", *WINDOWS[0])      # no filter: the native reader as ever
    be.read_filter = flt
    called = []
    orig = bamio.BamFile.chop_native
    monkeypatch.setattr(bamio.BamFile, "chop_native", lambda self, *a, **k: called.append(a) or orig(self, *a, **k))
    assert [be.chop(x, "c", a, b, fl) for a, b, fl in WINDOWS] == want
    assert [be.chop(x, "c", a, b, fl, right=True) for a, b, fl in WINDOWS] == want_r
    assert not called
    with pytest.raises(NotImplementedError):
        be.chop_many(x, ["c"], [9500], [10000], [500])
    with pytest.raises(NotImplementedError):
        be._open(x)._take_handle(L.load())


def test_every_handle_of_a_file_carries_the_filter(files):
    """BamFile opens a handle per call in flight: those that exist when the filter is set and those made later all apply it."""
    x, pre, _sites, _recs, _refs = files
    flt = FILTERS[0]
    lib = L.load()
    b = bamio.BamFile(x)
    first = [b._take_handle(lib) for _ in range(3)]
    with b._lock:
        b._free += first
    b.set_filter(*flt)
    held = [b._take_handle(lib) for _ in range(5)]          # three old ones, two new
    assert len(b._handles) == 5
    want = bamio.BamFile(pre[flt]).chop_native("c", *WINDOWS[0])
    tid, ch = b.tid["c"], b.index.chunks(b.tid["c"], WINDOWS[0][0] - 1, WINDOWS[0][1])
    for tl in held:
        assert b._chop_with(lib, tl, tid, ch, *WINDOWS[0]) == want
    with b._lock:
        b._free += held
    b.set_filter(0, 0)
    assert b.chop_native("c", *WINDOWS[0]) == bamio.BamFile(x).chop_native("c", *WINDOWS[0]) != want
    b.close()


# ------------------------------------------------------------------------------------------------------------------------------
# a record that stops a region today is rescued
# ------------------------------------------------------------------------------------------------------------------------------
def test_a_filtered_record_without_cigar_or_without_seq_stops_nothing(tmp_path, monkeypatch):
    rng = np.random.default_rng(8)
    ref = synth.random_dna(rng, 6000)
    good = []
    for i in range(6):
        a = 200 + 37 * i
        read, cig = synth.mutate(rng, ref[a:a + 3000])
        good.append(("g%d" % i, 0, a, cig, read, {"HP": 1 + i % 2, "PS": 4}, 60, 0))
    start, end, fl = 1000, 1600, 200
    # an unmapped mate placed at the window start, without CIGAR (the reference raises IndexError for the whole run, SF:331), and a
    # secondary record without SEQ (l_seq 0), which a window no longer than its miss_bp keeps as an empty read
    stop_c = ("mate", 0, start - 1, "*", "ACGT" * 50, None, 0, 0x4 | 0x1 | 0x40)
    stop_s = ("sec", 0, start - 1, "100M", "", None, 60, 0x100)
    refs = [("c", 6000)]
    clean, with_c, with_s = (str(tmp_path / n) for n in ("clean.bam", "nocigar.bam", "noseq.bam"))
    bamio.write_bam(clean, refs, good, block_size=BLOCK)
    bamio.write_bam(with_c, refs, good + [stop_c], block_size=BLOCK)
    bamio.write_bam(with_s, refs, good + [stop_s], block_size=BLOCK)
    ref_be = seqio.InProcessBam()
    for native in ("1", "0"):
        monkeypatch.setenv("VAPOR_BAM_NATIVE", native)
        be = seqio.InProcessBam()
        seqio.set_backend(be)
        for kw in ({}, {"tagged": True}, {"right": True}):
            want = ref_be.chop(clean, "c", start, end, fl, **kw)
            assert len(want) >= (0 if kw.get("right") else 6)
            be.read_filter = (0, 0)
            if not kw.get("right"):
                with pytest.raises(IndexError):
                    seqio.chop_pacbio_read_by_pos(with_c, "c", start, end, fl, **kw)
            be.read_filter = (0, 4)
            assert seqio.chop_pacbio_read_by_pos(with_c, "c", start, end, fl, **kw) == want
            be.read_filter = (0, 0x100)
            assert seqio.chop_pacbio_read_by_pos(with_s, "c", start, end, fl, **kw) == want
        # the degenerate window the record without SEQ is kept in today
        be.read_filter = (0, 0)
        today = be.chop(with_s, "c", start, start, fl)
        assert ["", 0, "sec"] in [r[:3] for r in today]
        be.read_filter = (0, 0x100)
        assert be.chop(with_s, "c", start, start, fl) == ref_be.chop(clean, "c", start, start, fl) == [r for r in today if r[2] != "sec"]
        if native == "1":
            be.read_filter = (0, 0)
            assert be.chop_many(with_c, ["c"], [start], [end], [fl])[4].tolist() == [-4]
            be.read_filter = (0, 4)
            assert _many(be, with_c, [(start, end, fl)]) == _many(ref_be, clean, [(start, end, fl)])
    seqio.set_backend(None)
    # the same through MemorySamtools and its array form
    wc = world_of(refs, good + [stop_c])
    mem, mem0 = seqio.MemorySamtools(wc), seqio.MemorySamtools(world_of(refs, good))
    with pytest.raises(IndexError):
        mem.chop("x", "c", start, end, fl)
    assert mem.chop_many("x", ["c"], [start], [end], [fl])[4].tolist() != [0]
    mem.read_filter = (0, 4)
    assert mem.chop("x", "c", start, end, fl) == mem0.chop("x", "c", start, end, fl)
    assert _many(mem, "x", [(start, end, fl)]) == _many(mem0, "x", [(start, end, fl)])


# ------------------------------------------------------------------------------------------------------------------------------
# end to end through cli.main
# ------------------------------------------------------------------------------------------------------------------------------
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
    if mode == "vcf":
        return seen["table"], (d / "in.vcf.vapor").read_text()
    return out.read_text(), None


MARKS_904 = ("mapq0", "mapq_low", "unmapped", "secondary", "supplementary")       # what --min-mapq 20 --exclude-flags 0x904 filters


def _hom_world(seed, svtypes=("DEL", "INV", "TANDUP")):
    """A true homozygous call (every read from the alternative haplotype) and a null call (every read from the contig) per type."""
    w = synth.make_world(seed=seed, n_loci=len(svtypes), svtypes=svtypes, span_range=(600, 900), read_len=2600, n_reads=5, alt_fraction=1.0)
    null = synth.make_world(seed=seed + 1, n_loci=len(svtypes), svtypes=svtypes, span_range=(600, 900), read_len=2600, n_reads=5,
                            alt_fraction=0.0, chrom_prefix="n")
    w.contigs.update(null.contigs)
    w.reads.update(null.reads)
    w.loci += null.loci
    return w


def _bnd_world():
    w = synth.make_bnd_world(41, forms=("3to5", "3to3"), n_reads=5)
    j = synth.make_junction_world(42, svtypes=("DEL", "INV"), n_reads=5)
    s = _hom_world(43, ("DEL",))
    for other in (j, s):
        w.contigs.update(other.contigs)
        w.reads.update(other.reads)
        w.loci += other.loci
    return w


def _vcf(w):
    simple = synth.SynthWorld()
    simple.loci = [l for l in w.loci if l.svtype != "BND"]
    return synth.vcf_text(simple, header=False) + synth.bnd_vcf_text(w)


FILTER_ARGS = ["--min-mapq", "20", "--exclude-flags", "0x904"]


def _three_runs(tmp_path, tag, w, d, mode, text, more, prepare=lambda: None):
    """(plain run on W, plain run on the decoy world, filtered run on the decoy world)."""
    out = []
    for name, world, extra in (("w", w, []), ("d", d, []), ("df", d, FILTER_ARGS)):
        seqio.set_backend(seqio.MemorySamtools(world))
        prepare()
        out.append(_main(tmp_path, tag + "_" + name, mode, text, list(more) + extra))
    return out


def _decoys_decide(clean, decoy, filtered):
    assert filtered == clean                                      # byte for byte: the table and, for vcf, the annotated VCF
    a, b = clean[0].splitlines(), decoy[0].splitlines()
    assert len(a) == len(b) and a[0] == b[0] and any(x != y for x, y in zip(a[1:], b[1:]))
    return sum(x != y for x, y in zip(a[1:], b[1:]))


def test_decoys_are_what_their_docstring_says():
    w = _hom_world(50)
    n0 = {c: list(r) for c, r in w.reads.items()}
    d = synth.add_decoys(w, 9)
    assert {c: list(r) for c, r in w.reads.items()} == n0 and d.contigs is w.contigs and d.loci is w.loci
    for c, recs in d.reads.items():
        own = [r for r in recs if not r.qname.startswith("d")]
        dec = [r for r in recs if r.qname.startswith("d")]
        assert own == w.reads[c] and len(dec) == 7
        assert sorted((r.mapq, r.flag) for r in dec) == sorted([(0, 0), (19, 0), (60, 4), (60, 0x100), (60, 0x200), (60, 0x400), (60, 0x800)])
        assert all(not passes(r.mapq, r.flag, 20, 0xF04) for r in dec) and all(passes(r.mapq, r.flag, 20, 0xF04) for r in own)
        # the other allele: a contig of alt reads gets reference decoys and the other way round
        assert {r.qname[-1] for r in dec} == ({"r"} if c.startswith("c") else {"a"}) != {r.qname[-1] for r in own}
        assert [r.cigar for r in dec if r.flag == 4] == ["*"] and [r.seq for r in dec if r.flag == 0x100] == [""]
    d5 = synth.add_decoys(w, 9, marks=MARKS_904)
    assert all(not passes(r.mapq, r.flag, 20, 0x904) for recs in d5.reads.values() for r in recs if r.qname.startswith("d"))
    # the decoys travel through the writer: the file holds their MAPQ and FLAG
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        _fa, bam = synth.write_world_files(d, tmp, block_size=2048)
        b = bamio.BamFile(bam)
        for c, recs in d.reads.items():
            got = b.fetch_lines(c, 1, len(d.contigs[c]))
            assert sorted(int(l.split("\t")[1]) for l in got) == sorted(r.flag for r in recs)
            b.set_filter(20, 0xF04)
            assert len(b.fetch_lines(c, 1, len(d.contigs[c]))) == len(w.reads[c])
            b.set_filter(0, 0)


@pytest.mark.parametrize("case", ["bed", "vcf_bnd", "refine", "phased", "phase_vcf", "both_ends"])
def test_the_decoy_world_with_the_filter_is_the_clean_world_without_it(fake, tmp_path, case):
    more, mode, prepare = [], "bed", (lambda: None)
    if case == "vcf_bnd":
        w, mode, more = _bnd_world(), "vcf", ["--bnd"]
    elif case == "both_ends":
        w, mode, more = _bnd_world(), "vcf", ["--bnd", "--both-ends"]
    elif case == "phased":
        w, more = synth.phase_world(_hom_world(61, ("DEL", "INV")), 5, untagged=0.1), ["--phased"]
    elif case == "phase_vcf":
        w = _hom_world(62, ("DEL", "INV"))
        snv = synth.snv_world(w, 6)
        p = tmp_path / "snv.vcf"
        p.write_text(synth.snv_vcf_text(snv))
        more = ["--phase-vcf", str(p)]
    elif case == "refine":
        w, more = _hom_world(63, ("DEL", "TANDUP")), ["--refine", "20"]
    else:
        w = _hom_world(60)
    d = synth.add_decoys(w, 17, marks=MARKS_904)
    text = _vcf(w) if mode == "vcf" else synth.bed_text(w)
    clean, decoy, filtered = _three_runs(tmp_path, case, w, d, mode, text, more, prepare)
    n = _decoys_decide(clean, decoy, filtered)
    print(case, "rows the decoys change:", n, "of", len(clean[0].splitlines()) - 1)
    if case == "bed":
        # Q = 0 and F = 0 given explicitly are the options left out; all seven marks against 0xF04
        seqio.set_backend(seqio.MemorySamtools(d))
        assert _main(tmp_path, "zero", "bed", text, ["--min-mapq", "0", "--exclude-flags", "0x0"]) == decoy
        seqio.set_backend(seqio.MemorySamtools(synth.add_decoys(w, 17)))
        assert _main(tmp_path, "all7", "bed", text, ["--min-mapq", "20", "--exclude-flags", "0xF04"]) == clean
        assert _main(tmp_path, "all7_904", "bed", text, FILTER_ARGS) != clean      # (0x200 and 0x400 are not in 0x904)


def test_an_unmapped_mate_on_a_window_start_ends_the_plain_run_and_not_the_filtered_one(fake, tmp_path):
    """add_decoys(stoppers=2): the FLAG-4 decoys of two loci lie on the start of their read windows.  The plain run on that world
    ends in the reference's IndexError; with the filter the table is the clean world's, byte for byte - bed and vcf."""
    w = _hom_world(64)
    d = synth.add_decoys(w, 19, marks=MARKS_904, stoppers=2)
    moved = [r for recs in d.reads.values() for r in recs if r.flag == 4 and r.cigar == "*"
             and any(l.chrom == r.rname and r.pos == l.start - min(500, l.end - l.start) for l in w.loci)]
    assert len(moved) == 2
    for mode, text in (("bed", synth.bed_text(w)), ("vcf", synth.vcf_text(w, header=False))):
        seqio.set_backend(seqio.MemorySamtools(w))
        clean = _main(tmp_path, "stop_w_" + mode, mode, text)
        seqio.set_backend(seqio.MemorySamtools(d))
        with pytest.raises(IndexError):
            _main(tmp_path, "stop_d_" + mode, mode, text)
        assert _main(tmp_path, "stop_df_" + mode, mode, text, FILTER_ARGS) == clean
        assert _main(tmp_path, "stop_d4_" + mode, mode, text, ["--exclude-flags", "4"]) != clean      # (the other decoys still vote)


def test_phased_majority_phase_set_follows_the_filtered_records(fake, tmp_path):
    """A window whose majority phase set flips when its MAPQ-0 records are dropped: VaPoR_PS and the nine columns are those of
    the world without them."""
    w = synth.make_world(seed=70, n_loci=1, svtypes=("DEL",), span_range=(700, 800), read_len=2600, n_reads=9, alt_fraction=1.0)
    recs = w.reads["c1"]
    for i, r in enumerate(recs):
        if i < 5:
            r.tags, r.mapq = {"HP": 1, "PS": 7}, 0              # five placements inside a duplication: phase set 7
        else:
            r.tags = {"HP": 1 + i % 2, "PS": 9}                 # four unique ones: phase set 9
    clean = synth.SynthWorld()
    clean.contigs, clean.loci, clean.reads = w.contigs, w.loci, {"c1": [r for r in recs if r.mapq]}
    bed = synth.bed_text(w)
    seqio.set_backend(seqio.MemorySamtools(w))
    plain, _ = _main(tmp_path, "plain", "bed", bed, ["--phased"])
    filt, _ = _main(tmp_path, "filt", "bed", bed, ["--phased", "--min-mapq", "1"])
    seqio.set_backend(seqio.MemorySamtools(clean))
    want, _ = _main(tmp_path, "want", "bed", bed, ["--phased"])
    head = plain.splitlines()[0].split("\t")
    col = head.index("VaPoR_PS")
    assert len(head) - col == 9
    assert plain.splitlines()[1].split("\t")[col] == "7" and filt.splitlines()[1].split("\t")[col] == "9"
    assert filt == want != plain


# ------------------------------------------------------------------------------------------------------------------------------
# the writer, and the host reader under sanitizers
# ------------------------------------------------------------------------------------------------------------------------------
def _writer_records():
    rng = np.random.default_rng(20260)
    ref = synth.random_dna(rng, 20000)
    recs = []
    for i in range(40):
        a = int(rng.integers(0, 16000))
        read, cig = synth.mutate(rng, ref[a:a + int(rng.integers(200, 1500))])
        if i % 5 == 1:
            cig, read = "12S" + cig, "ACGTACGTACGT" + read
        tags = {"HP": 1 + i % 2, "PS": 7} if i % 3 == 0 else None
        recs.append(("w%d" % i, i % 2, a, cig, read) + ((tags,) if tags else ()))
    return [("c", 20000), ("d", 20000)], recs


def test_writer_without_the_new_fields_writes_the_bytes_it_wrote_before(tmp_path):
    """The sha256 values are those of the files the writer made from these records before it took MAPQ and FLAG."""
    refs, recs = _writer_records()
    out = str(tmp_path / "w.bam")
    bamio.write_bam(out, refs, recs, block_size=3000)
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == "f7bd6de8be940f18fa0a8dd61c395fc49531bb8c8343aeae48ee2bde148cdd20"
    assert hashlib.sha256(open(out + ".bai", "rb").read()).hexdigest() == "29610d75fea2988a422fc9e62ede4286a7ea69de7b5e1052ad5b022f9b8ae023"
    bamio.write_bam(out, refs, recs, block_size=3000, qual_seed=5)
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == "b78179d9944274d75f600c7f64c5738a57253fd11a705566f76b671d172d0a26"
    # the defaults spelled out, and None, are the same bytes; other values are the two fields alone
    full = [tuple(r[:5]) + ((r[5] if len(r) > 5 else None), 60, 0) for r in recs]
    bamio.write_bam(out, refs, full, block_size=3000, qual_seed=5)
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == "b78179d9944274d75f600c7f64c5738a57253fd11a705566f76b671d172d0a26"
    bamio.write_bam(out, refs, [tuple(r[:5]) + ((r[5] if len(r) > 5 else None), None, None) for r in recs], block_size=3000, qual_seed=5)
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == "b78179d9944274d75f600c7f64c5738a57253fd11a705566f76b671d172d0a26"
    marked = [r[:6] + (i % 256, (i * 997) % 65536) for i, r in enumerate(full)]
    bamio.write_bam(out, refs, marked, block_size=3000)
    b = bamio.BamFile(out)
    seen = {}
    cur = b.bgzf.read_from(b.first_record)
    while True:
        hdr = cur.read(4)
        if len(hdr) < 4:
            break
        rec = cur.read(int.from_bytes(hdr, "little"))
        _ref_id, _pos, name, flag, _cig, _l_seq, _sq, _tags, mapq = bamio.BamFile._parse(rec)
        seen[name] = (mapq, flag)
    assert seen == {r[0]: (r[6], r[7]) for r in marked}
    for bad in ((256, 0), (-1, 0), (0, 65536)):
        with pytest.raises(ValueError):
            bamio.write_bam(out, refs, [full[0][:6] + bad])


def test_native_reader_with_a_filter_under_sanitizers(files, tmp_path):
    """tools/bam_check.cpp (a stand-alone program) built with AddressSanitizer and UBSan, run over the files of this module with a
    filter: exit 0, no report, and the reads it counts are those of the prefiltered file; without the two arguments it prints what
    it printed before."""
    x, pre, _sites, _recs, _refs = files
    exe = str(tmp_path / "bam_check")
    cmd = ["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "vapor_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tools", "bam_check.cpp"), "-lz", "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(path, win, *more):
        first = bamio.BamFile(path).first_record
        p = subprocess.run([exe, path, str(first), "0", str(win[0]), str(win[1]), str(win[2]), "2"] + [str(m) for m in more], env=env,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, (path, p.returncode, p.stderr[-2000:])
        return p.stdout.splitlines()
    n_reads = 0
    for flt in FILTERS:
        for win in WINDOWS[:3]:
            got = run(x, win, flt[0], hex(flt[1]))
            want = run(pre[flt], win, 0, 0)
            assert got[0] == "filter: rc 0 " and got[1:] == want[1:] and len(got) >= 4, (flt, win, got, want)
            plain = run(x, win)
            assert not any(l.startswith(("filter", "right", "tagged")) for l in plain)
            n_reads += int(got[-1].split("reads ")[1].split()[0])
    assert n_reads > 0
    assert run(x, WINDOWS[0], 256, 0)[0].startswith("filter: rc -4")

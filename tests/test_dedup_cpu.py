"""`--dedup-qname` on the host.  The reference has no such rule, so the statement tested against is the
definition: reading file X with the option equals reading, without it, the file written from X minus the records rule W drops -
per route (the Python statement, the four native readers, MemorySamtools, SAM text), on records designed case by case with the
dropped ones named by hand; the name key against hand-computed values and against csrc/vapor_names.h under the sanitizers
(tools/names_check.cpp); rule V of `--both-ends` through cli.main on split-alignment worlds (synth.add_split_alignments) against a
pool made by hand from the views and their keys.  Device work is answered by tests/fake_engine.py (oracle-backed, test only)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from fake_engine import FakeEngine
from vapor_amd import _lib as L
from vapor_amd import bamio, bothends, cli, finish, modes, phase, pipeline, seqio, synth
from vapor_amd import simple_function as SF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1


@pytest.fixture()
def fake(oracle):
    pipeline.set_engine(FakeEngine(oracle))
    yield
    pipeline.set_engine(None)
    seqio.set_backend(None)


# ------------------------------------------------------------------------------------------------------------------------------
# the name key
# ------------------------------------------------------------------------------------------------------------------------------
def fin(z):
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def test_name_key_against_hand_computed_values():
    # "": h = 0, and the finaliser maps 0 to 0
    assert seqio.name_key("") == 0
    # "a": h = 1 + (0x61 + 1) * M
    assert (1 + 98 * M) & MASK == 0x913C9902BA83800B and seqio.name_key("a") == fin(0x913C9902BA83800B) == 0xD80391FFB30D1390
    # "ab": h = 2 + 98 * M + 99 * M^2
    assert (2 + 98 * M + 99 * M * M) & MASK == 0xE89A0D78807E3297 and seqio.name_key("ab") == fin(0xE89A0D78807E3297) == 0xA2595B259536A26E
    # a prefix is another name: the length is part of h, and the new byte's term is not zero (b + 1 >= 1, M odd)
    assert seqio.name_key("abc") == 0x9C4F06DE828618C2 != seqio.name_key("ab")
    assert seqio.name_key("abc") == fin((3 + 98 * M + 99 * M ** 2 + 100 * M ** 3) & MASK)
    # 254 bytes, the longest name a BAM record holds
    assert seqio.name_key("q" * 254) == 0x604217B4F56993F6 == fin((254 + sum(114 * pow(M, i + 1, 1 << 64) for i in range(254))) & MASK)
    assert seqio.name_key(bytes(range(1, 255))) == 0x00B68FDF16B264DC
    # bytes and text are one name; a NUL byte counts (b + 1)
    assert seqio.name_key(b"read/1") == seqio.name_key("read/1") and seqio.name_key(b"\0") != seqio.name_key(b"") != seqio.name_key(b"\0\0")
    # one byte changed never collides
    base = bytearray(b"m64011_190830_220126/1234/ccs")
    keys = {seqio.name_key(bytes(base))}
    for i in range(len(base)):
        for d in (1, 2, 128, 255):
            other = bytearray(base)
            other[i] = (other[i] + d) & 255
            keys.add(seqio.name_key(bytes(other)))
    assert len(keys) == 1 + 4 * len(base)


@pytest.fixture(scope="module")
def names_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("names")
    exe = str(d / "names_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "vapor_amd", "csrc"), os.path.join(ROOT, "tools", "names_check.cpp"), "-o", exe])
    rng = np.random.default_rng(5)
    names = [b"", b"a", b"ab", b"abc", b"q" * 254, bytes(range(1, 255))]
    for n in (1, 3, 4, 5, 63, 64, 65, 200, 253, 254):
        names.append(bytes(rng.integers(33, 127, n).astype(np.uint8)))
        names.append(bytes(rng.integers(1, 256, n).astype(np.uint8)))
    src = d / "names.txt"
    src.write_text("".join(n.hex() + "\n" for n in names))
    r = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return names, r.stdout


def test_native_name_key_and_drop_rule_under_sanitizers(names_check):
    """The stand-alone program includes csrc/vapor_names.h - the header bam_dedup_kernel and the host reader include - and holds
    name_key to the sum of the 64 lanes' terms and the drop predicate to its O(n^2) statement (0, 1, 2, 64, 65, 256 entries); the
    keys it prints for these names are seqio.name_key's."""
    names, out = names_check
    for line in ("table: 257 powers", "name_key: 2040 names equal the lanes' sum", "drops: 1200 arrays equal the direct statement",
                 "names_check: all equal"):
        assert line in out
    got = [int(l.split()[1], 16) for l in out.splitlines() if l.startswith("key ")]
    assert got == [seqio.name_key(n) for n in names] and len(got) == len(names) == 26


def test_rule_w_in_python_names_the_survivor():
    mask = seqio.dedup_mask
    assert mask([], []) == [] and mask(["a"], [0x900]) == [True]
    assert mask(["a", "a"], [0x800, 0]) == [False, True]                       # supplementary first: the primary survives
    assert mask(["a", "a"], [0x100, 0x100]) == [True, False]                   # two secondaries: the first
    assert mask(["a", "b", "a", "a"], [0x800, 0, 0, 0]) == [False, True, True, False]
    assert mask(["a", "a"], [0x10, 0x400]) == [True, False]                    # other FLAG bits decide nothing
    assert mask(["a", "a", "a"], [0x100, 0x800, 0x900]) == [True, False, False]


# ------------------------------------------------------------------------------------------------------------------------------
# rule W per route: designed records, the dropped ones named by hand
# ------------------------------------------------------------------------------------------------------------------------------
CONTIG = 48000
BLOCK = 900
FLANK = 500


def _base(k):
    return 6000 * k + 3000          # case k's window is [base, base + 1000], its loci anchor base + 500


# per case: (name, POS offset from the window start, FLAG, MAPQ, tags, deletion before the window start or 0), in file order, and
# the indices rule W drops
CASES = {
    "supp_first": ([("m0", -600, 0x800, 60, None, 0), ("o0", -580, 0, 60, None, 0), ("m0", -550, 0, 60, None, 0)], {0}),
    "two_secondaries": ([("m1", -600, 0x100, 60, None, 0), ("m1", -590, 0x100, 60, None, 0), ("o1", -500, 0, 60, None, 0)], {1}),
    "three": ([("m2", -700, 0x800, 60, None, 0), ("m2", -650, 0, 60, None, 0), ("x2", -640, 0, 60, None, 0),
               ("m2", -600, 0, 60, None, 0)], {0, 3}),
    # 20 molecules, every third with miss_bp > 0, and a secondary twin of d5 with miss_bp 0: 21 kept records are cut to 20 by
    # miss_bp, 20 are the list as it lies
    "over_20": ([("d%d" % i, -900 + 10 * i, 0, 60, None, 12 + i if i % 3 == 1 else 0) for i in range(20)]
                + [("d5", -690, 0x100, 60, None, 0)], {20}),
    # phase set 7 has four tagged records but two molecules, phase set 9 three of three: the majority flips
    "phase_flip": ([("p0", -700, 0, 60, {"HP": 1, "PS": 7}, 0), ("p0", -690, 0x100, 60, {"HP": 1, "PS": 7}, 0),
                    ("p1", -680, 0, 60, {"HP": 1, "PS": 7}, 0), ("p1", -670, 0x800, 60, {"HP": 1, "PS": 7}, 0),
                    ("r0", -660, 0, 60, {"HP": 2, "PS": 9}, 0), ("r1", -650, 0, 60, {"HP": 1, "PS": 9}, 0),
                    ("r2", -640, 0, 60, {"HP": 2, "PS": 9}, 0)], {1, 3}),
    # with --min-mapq 20 the primary is not in the file: the first of the two others survives
    "filtered_survivor": ([("f0", -600, 0, 5, None, 0), ("f0", -590, 0x800, 60, None, 0), ("f0", -580, 0x100, 60, None, 0),
                           ("g0", -570, 0, 60, None, 0)], {2}),
}
ORDER = list(CASES)
FILTER_OF = {"filtered_survivor": (20, 0)}


def designed(seed=3):
    """(refs, all records, the records without the dropped ones, sites): every read an exact copy of the contig from its POS to
    600 bases behind the window end - both anchor kinds keep it - some with a deletion that straddles the window start."""
    rng = np.random.default_rng(seed)
    ref = synth.random_dna(rng, CONTIG)
    full, rest = [], []
    for k, name in enumerate(ORDER):
        recs, dropped = CASES[name]
        b0 = _base(k) - 1                                   # 0-based window start
        for i, (q, off, flag, mapq, tags, dele) in enumerate(recs):
            a, e = b0 + off, b0 + 1000 + 600
            if dele:
                left = b0 - 5 - a                           # aligned up to five bases before the window start, then the deletion
                cig, seq = "%dM%dD%dM" % (left, dele, e - (a + left + dele)), ref[a:a + left] + ref[a + left + dele:e]
            else:
                cig, seq = "%dM" % (e - a), ref[a:e]
            rec = (q, 0, a, cig, seq, tags, mapq, flag)
            full.append(rec)
            if i not in dropped:
                rest.append(rec)
    sites = []
    for k in range(len(ORDER)):
        for p in range(_base(k) - 400, _base(k) + 1400, 91):
            r = ref[p - 1]
            alt = "ACGT"[("ACGT".index(r) + 1 + p % 3) % 4]
            sites.append(("c", p, r, alt, 5) if p % 2 else ("c", p, alt, r, 6))
    return [("c", CONTIG)], full, rest, phase.Sites.from_rows(sites)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("dd")
    refs, full, rest, sites = designed()
    x, p = str(d / "x.bam"), str(d / "p.bam")
    bamio.write_bam(x, refs, full, block_size=BLOCK)
    bamio.write_bam(p, refs, rest, block_size=BLOCK)
    return x, p, sites, refs, full, rest


def world_of(refs, recs):
    w = synth.SynthWorld()
    for name, n in refs:
        w.contigs[name] = "A" * n
        w.reads[name] = []
    for qname, tid, pos0, cig, seq, tags, m, f in sorted(recs, key=lambda r: (r[1], r[2])):
        span = sum(int(k) for k, op in seqio._CIGAR_RE.findall(cig) if op in "MDN=X")
        w.reads[refs[tid][0]].append(synth.SamRecord(qname, refs[tid][0], pos0 + 1, cig, seq, max(span, 1), tags, f, m))
    return w


def _many(be, src, regions, **kw):
    got = be.chop_many(src, ["c"] * len(regions), [r[0] for r in regions], [r[1] for r in regions], [r[2] for r in regions], **kw)
    kf, addr, q0, miss, status = got[:5]
    reads = [[ctypes.string_at(int(addr[t]) + int(q0[t]), r[1] - r[0] - int(miss[t])).decode() for t in range(int(kf[g]), int(kf[g + 1]))]
             for g, r in enumerate(regions)]
    rest = [np.asarray(a).tolist() for a in got[6:]]
    return np.diff(kf).tolist(), reads, miss.tolist(), status.tolist(), rest


def _windows(name):
    b = _base(ORDER.index(name))
    return (b, b + 1000, FLANK)


def test_the_designed_file_is_what_its_cases_say(files):
    """Without the option every record of a case is kept by both anchor kinds; the cases' dropped records are exactly those the
    rule names on (QNAME, FLAG) in file order."""
    x, p, _sites, _refs, full, rest = files
    be = seqio.InProcessBam()
    for name in ORDER:
        recs, dropped = CASES[name]
        for kw in ({}, {"right": True}):
            assert [r[2] for r in be.chop(x, "c", *_windows(name), **kw)] == [r[0] for r in recs]
            assert [r[2] for r in be.chop(p, "c", *_windows(name), **kw)] == [r[0] for i, r in enumerate(recs) if i not in dropped]
        q, f = FILTER_OF.get(name, (0, 0))
        seen = [(r[0], r[2]) for r in recs if bamio.record_passes(r[3], r[2], q, f)]
        live = seqio.dedup_mask([s[0] for s in seen], [s[1] for s in seen])
        assert [s for s, ok in zip(seen, live) if not ok] == [(recs[i][0], recs[i][2]) for i in sorted(dropped)]
    assert len(full) - len(rest) == 8


@pytest.mark.parametrize("name", ORDER)
def test_file_routes_read_x_with_the_option_as_the_file_without_the_dropped_records(files, name, monkeypatch):
    """chop_python, vapor_bam_chop, _tagged, _haplotag, _right and chop_many: entry by entry read, miss_bp, qname, hap, ps."""
    x, p, sites, _refs, _full, _rest = files
    monkeypatch.delenv("VAPOR_BAM_NATIVE", raising=False)
    bx, bp, plain = seqio.InProcessBam(), seqio.InProcessBam(), seqio.InProcessBam()
    bx.dedup_qname = True
    bx.read_filter = bp.read_filter = plain.read_filter = FILTER_OF.get(name, (0, 0))
    win = _windows(name)
    for kw in ({}, {"tagged": True}, {"tagged": True, "sites": sites}):
        want = bp.chop_python(p, "c", *win, **kw)
        assert bx.chop_python(x, "c", *win, **kw) == want and want
        assert bx.chop(x, "c", *win, **kw) == want and bp.chop(p, "c", *win, **kw) == want
        assert plain.chop(x, "c", *win, **kw) != want                       # (the option decides something in every case)
    want = bp.chop(p, "c", *win, right=True)
    assert bx.chop(x, "c", *win, right=True) == want and plain.chop(x, "c", *win, right=True) != want
    monkeypatch.setenv("VAPOR_BAM_NATIVE", "0")
    assert bx.chop(x, "c", *win, right=True) == want and bx.chop(x, "c", *win) == bp.chop(p, "c", *win)
    monkeypatch.delenv("VAPOR_BAM_NATIVE")
    for kw in ({}, {"groups": True}, {"groups": True, "sites": sites}, {"max_keep": 3}):
        assert _many(bx, x, [win], **kw) == _many(bp, p, [win], **kw)
    # the lists the drivers take: minimize_pacbio_read_list and phase.select behind the rule
    for be, src in ((bx, x), (bp, p), (plain, x)):
        seqio.set_backend(be)
        be.lists = (seqio.simple_del_chop_pacbio_read_simple_short(src, ["c", win[0] + FLANK], FLANK),
                    seqio.simple_del_chop_pacbio_read_simple_short(src, ["c", -(win[0] + FLANK)], FLANK, right=True))
        sel = seqio.simple_del_chop_pacbio_read_simple_short(src, ["c", win[0] + FLANK], FLANK, phased=True)
        be.sel = (list(sel), sel.tagged, sel.ps, [list(g) for g in sel.groups])
    seqio.set_backend(None)
    assert bx.lists == bp.lists and bx.sel == bp.sel
    if name == "over_20":
        # 21 kept records are cut by miss_bp, 20 are the list as it lies: the duplicate would have pushed the list over 20
        assert len(plain.lists[0]) == 20 == len(bx.lists[0]) and plain.lists[0] != bx.lists[0]
        assert [r[2] for r in bx.lists[0]] == ["d%d" % i for i in range(20)]
        assert sorted(r[1] for r in plain.lists[0]) == [r[1] for r in plain.lists[0]] != [r[1] for r in bx.lists[0]]
    if name == "phase_flip":
        assert plain.sel[2] == 7 and bx.sel[2] == 9 and plain.sel[1] and bx.sel[1]
        assert _many(plain, x, [win], groups=True)[4][1] == [7] and _many(bx, x, [win], groups=True)[4][1] == [9]


@pytest.mark.parametrize("name", ORDER)
def test_memory_and_text_routes_read_the_world_with_the_option_as_the_world_without_the_dropped_records(files, name, monkeypatch):
    _x, p, sites, refs, full, rest = files
    wx, wp = world_of(refs, full), world_of(refs, rest)
    mx, mp = seqio.MemorySamtools(wx), seqio.MemorySamtools(wp)
    mx.dedup_qname = True
    flt = FILTER_OF.get(name, (0, 0))
    mx.read_filter = mp.read_filter = flt

    class Text:                      # a backend that answers in SAM text alone, as the samtools binary's does
        read_filter = flt
        dedup_qname = True
        view_lines = seqio.MemorySamtools(wx).view_lines

    class TextPre:
        read_filter = flt
        view_lines = seqio.MemorySamtools(wp).view_lines
    win = _windows(name)
    for kw in ({}, {"tagged": True}, {"tagged": True, "sites": sites}, {"right": True}):
        want = mp.chop("x", "c", *win, **kw)
        assert mx.chop("x", "c", *win, **kw) == want and want
        monkeypatch.setenv("VAPOR_MEMORY_CHOP", "records")
        assert mx.chop("x", "c", *win, **kw) == want
        monkeypatch.delenv("VAPOR_MEMORY_CHOP")
        seqio.set_backend(Text())
        got = seqio.chop_pacbio_read_by_pos("x", "c", *win, **kw)
        seqio.set_backend(TextPre())
        assert got == seqio.chop_pacbio_read_by_pos("x", "c", *win, **kw) == want
        seqio.set_backend(None)
    for kw in ({}, {"groups": True}, {"groups": True, "sites": sites}, {"max_keep": 3}):
        assert _many(mx, "x", [win], **kw) == _many(mp, "x", [win], **kw)
    # the option set later, or taken back, is what is applied
    mx.dedup_qname = False
    full_be = seqio.MemorySamtools(wx)
    full_be.read_filter = flt
    assert _many(mx, "x", [win]) == _many(full_be, "x", [win]) != _many(mp, "x", [win])
    # the files and the worlds hold the same records: the two families agree with each other
    fb = seqio.InProcessBam()
    fb.read_filter = flt
    assert [r[:3] for r in mp.chop("x", "c", *win)] == [r[:3] for r in fb.chop(p, "c", *win)]


def test_a_library_without_the_entry_sends_a_deduplicating_run_through_the_python_statement(files, monkeypatch):
    x, p, _sites, _refs, _full, _rest = files
    real = L.load()

    class Without:
        def __getattr__(self, name):
            if name in ("vapor_bam_set_dedup", "vapor_bam_batch_name_keys"):
                raise AttributeError(name)
            return getattr(real, name)
    bp = seqio.InProcessBam()
    wins = [_windows(n) for n in ORDER if n not in FILTER_OF]
    want = [bp.chop(p, "c", *w) for w in wins]
    want_r = [bp.chop(p, "c", *w, right=True) for w in wins]
    for name in ("vapor_bam_set_dedup", "vapor_bam_batch_name_keys"):
        assert name in L.EXPORTS and name in L.OPTIONAL_EXPORTS
    assert L.ABI_VERSION == 3
    monkeypatch.setattr(L, "_lib", Without())
    be = seqio.InProcessBam()
    assert be.chop(x, "c", *wins[0]) == seqio.InProcessBam().chop(x, "c", *wins[0])        # option off: the native reader as ever
    be.dedup_qname = True
    assert not be._open(x).native_dedup_ok() and seqio.InProcessBam()._open(x).native_dedup_ok()
    called = []
    orig = bamio.BamFile.chop_native
    monkeypatch.setattr(bamio.BamFile, "chop_native", lambda self, *a, **k: called.append(a) or orig(self, *a, **k))
    assert [be.chop(x, "c", *w) for w in wins] == want and [be.chop(x, "c", *w, right=True) for w in wins] == want_r
    assert not called
    with pytest.raises(NotImplementedError):
        be.chop_many(x, ["c"], [wins[0][0]], [wins[0][1]], [FLANK])
    with pytest.raises(NotImplementedError):
        be.chop_many_device(object(), x, ["c"], [wins[0][0]], [wins[0][1]], [FLANK])
    with pytest.raises(NotImplementedError):
        be._open(x)._take_handle(L.load())


def test_every_handle_of_a_file_carries_the_option_and_bad_values_are_refused(files):
    x, p, _sites, _refs, _full, _rest = files
    lib = L.load()
    b = bamio.BamFile(x)
    win = _windows("three")
    first = [b._take_handle(lib) for _ in range(2)]
    with b._lock:
        b._free += first
    b.set_dedup(True)
    held = [b._take_handle(lib) for _ in range(3)]          # two old ones, one new
    want = bamio.BamFile(p).chop_native("c", *win)
    tid, ch = b.tid["c"], b.index.chunks(b.tid["c"], win[0] - 1, win[1])
    for tl in held:
        assert b._chop_with(lib, tl, tid, ch, *win) == want
    h = held[0]["native"]
    for bad in (2, -1, 256):
        assert lib.vapor_bam_set_dedup(h, bad) == L.E_ARG
    assert b._chop_with(lib, held[0], tid, ch, *win) == want                               # (a refused value changes nothing)
    with b._lock:
        b._free += held
    b.set_dedup(False)
    assert b.chop_native("c", *win) == bamio.BamFile(x).chop_native("c", *win) != want
    b.close()


def test_native_reader_with_small_buffers_sizes_the_second_call(files):
    """vapor_bam_chop with buffers too small answers VAPOR_E_OVERFLOW and sizes that hold all kept records; the call with those
    buffers returns the survivors."""
    x, p, _sites, _refs, _full, _rest = files
    lib = L.load()
    b = bamio.BamFile(x)
    b.set_dedup(True)
    tl = b._take_handle(lib)
    tl["buf"] = {"seq": np.empty(64, dtype=np.uint8), "names": ctypes.create_string_buffer(8), "meta": np.empty(4, dtype=np.int64),
                 "need": np.zeros(3, dtype=np.int64)}
    win = _windows("over_20")
    tid, ch = b.tid["c"], b.index.chunks(b.tid["c"], win[0] - 1, win[1])
    assert b._chop_with(lib, tl, tid, ch, *win) == bamio.BamFile(p).chop_native("c", *win)
    assert int(tl["buf"]["need"][2]) == 20 and tl["buf"]["seq"].size > 64          # (the sizes of the call that succeeded: the survivors')
    with b._lock:
        b._free.append(tl)
    b.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the parser and the backend
# ------------------------------------------------------------------------------------------------------------------------------
BASE = ["--reference", "r", "--pacbio-input", "b", "--no-figures"]


@pytest.mark.parametrize("cmd", ["bed", "vcf", "svelter", "ins"])
def test_all_four_subcommands_take_the_option_and_set_the_backend_once(cmd, tmp_path, monkeypatch):
    from vapor_amd import melt
    src = tmp_path / ("in." + ("vcf" if cmd == "vcf" else "bed"))
    src.write_text("")
    be = seqio.MemorySamtools(synth.SynthWorld())
    seqio.set_backend(be)
    seen = []
    monkeypatch.setattr(cli, "score_jobs", lambda jobs, *a, **k: seen.append(seqio.get_backend().dedup_qname) or [])
    monkeypatch.setattr(melt, "run", lambda *a, **k: seen.append(seqio.get_backend().dedup_qname))
    monkeypatch.setattr(SF, "vcf_vapor_modify", lambda *a, **k: None)
    args = [cmd, "--sv-input", str(src), "--output-path", str(tmp_path / "figs"), "--output-file", str(tmp_path / "out")] + BASE
    try:
        assert cli.build_parser().parse_args(args[1:]).dedup_qname is False and cli.build_parser().parse_args(args[1:] + ["--dedup-qname"]).dedup_qname is True
        assert cli.main(args) == 0
        assert cli.main(args + ["--dedup-qname"]) == 0
        assert cli.main(args + ["--dedup-qname", "--min-mapq", "20", "--exclude-flags", "0x704"]) == 0
        assert cli.main(args) == 0
        assert seen == [False, True, True, False] and be.dedup_qname is False and be.read_filter == (0, 0)
    finally:
        seqio.set_backend(None)


# ------------------------------------------------------------------------------------------------------------------------------
# rule V: the pooled columns of --both-ends
# ------------------------------------------------------------------------------------------------------------------------------
def _main(tmp_path, name, mode, text, more=()):
    d = tmp_path / name
    d.mkdir()
    src = d / ("in." + mode)
    src.write_text(text)
    out = d / "out.vapor"
    args = [mode, "--sv-input", str(src), "--reference", "ref.fa", "--pacbio-input", "x.bam", "--output-path", str(d / "figs"),
            "--output-file", str(out), "--no-figures"] + (["--bnd"] if mode == "vcf" else []) + list(more)
    seen = {}
    orig = SF.vcf_vapor_modify
    orig_cols = modes.BOTH_ENDS.columns_many

    def keep_table(vcf_input, rec_new, *a, **k):
        seen["table"] = open(vcf_input + ".vapor").read()
        return orig(vcf_input, rec_new, *a, **k)

    def keep_views(views_list):
        seen["views"] = list(views_list)
        return orig_cols(views_list)
    SF.vcf_vapor_modify = keep_table
    modes.BOTH_ENDS.columns_many = keep_views
    try:
        assert cli.main(args) == 0
    finally:
        SF.vcf_vapor_modify = orig
        modes.BOTH_ENDS.columns_many = orig_cols
    table = seen["table"] if mode == "vcf" else out.read_text()
    return [r.split("\t") for r in table.splitlines()], seen.get("views")


def _hand_pool(views, keys):
    """Rule V, stated here: the scored views in table order; a score is skipped when its read's key belongs to a read that
    contributed a score in an earlier scored view."""
    pooled, earlier = [], set()
    for v, ks in zip(views, keys):
        if v is None:
            continue
        assert len(v) == len(ks)
        mine = []
        for s, k in zip(v, ks):
            if k not in earlier:
                pooled.append(s)
                mine.append(k)
        earlier.update(mine)
    return pooled


def _vcf_of(w):
    return synth.bnd_vcf_text(w)


@pytest.mark.parametrize("mode", ["bed", "vcf"])
def test_pooled_columns_count_a_molecule_once_across_views(fake, tmp_path, mode):
    if mode == "bed":
        base = synth.make_junction_world(3, ("DEL", "TANDUP"), ref_fraction=0.0)
        text = synth.bed_text(base)
    else:
        base = synth.make_bnd_world(2, ("3to5", "3to5"))
        text = _vcf_of(base)
    full = synth.add_split_alignments(base, "full", window_dups=0)
    hard = synth.add_split_alignments(base, "hard", window_dups=0)
    assert full.planted["split"] > 0 and hard.planted["split"] == full.planted["split"]
    runs = {}
    for tag, w, more in (("w", full, ["--dedup-qname"]), ("off", full, []), ("hard_on", hard, ["--dedup-qname"]), ("hard_off", hard, []),
                         ("base_on", base, ["--dedup-qname"]), ("base_off", base, [])):
        seqio.set_backend(seqio.MemorySamtools(w))
        runs[tag] = _main(tmp_path, tag, mode, text, ["--both-ends"] + more)
    rows, views = runs["w"]
    rows_off, views_off = runs["off"]
    assert rows[0][-7:] == list(bothends.COLUMNS)
    be0 = len(rows[1]) - 7                                  # (the seven close every row, the row's own five lie before them)
    own0 = be0 - 5
    skipped = 0
    junction_rows = 0
    for r, r_off, v, v_off in zip(rows[1:], rows_off[1:], views, views_off):
        if v is None:
            assert r[be0:] == ["."] * 7
            continue
        junction_rows += 1
        assert v.keys is not None and getattr(v_off, "keys", None) is None
        pooled = _hand_pool(v, v.keys)
        cat = [s for x in v if x is not None for s in x]
        skipped += len(cat) - len(pooled)
        assert r[be0] == str(sum(1 for x in v if x is not None))
        assert r[be0 + 1:be0 + 6] == [str(x) for x in finish.row_tail(pooled)]
        # VaPoR_BE_SQS and the row's own columns: rule W alone makes them - no record of one name lies twice in one window of
        # these worlds, so they are the run's without the option
        assert r[be0 + 6] == ",".join("." if x is None else str(finish.row_tail(x)[0]) for x in v) == r_off[be0 + 6]
        assert r[own0:be0] == r_off[own0:be0] == [str(x) for x in finish.row_tail(v[0] or [])]
        assert [None if x is None else list(x) for x in v] == [None if x is None else list(x) for x in v_off]
        # the keys are the reads' names' keys: every key of a view is one molecule of the world
        names = {seqio.name_key(q.qname) for rs in full.reads.values() for q in rs}
        assert all(k in names for ks in v.keys if ks is not None for k in ks)
    assert junction_rows >= 2 and skipped > 0
    # without rule V the same molecules count twice: the pooled columns differ
    assert any(a[be0 + 1:be0 + 6] != b[be0 + 1:be0 + 6] for a, b in zip(rows[1:], rows_off[1:]))
    # hard-clipped supplementaries are too short for any view: nothing changes, with or without the option
    assert runs["hard_on"][0] == runs["hard_off"][0] == runs["base_off"][0]
    # a world without shared QNAMEs: the option changes no byte
    assert runs["base_on"][0] == runs["base_off"][0]


def test_window_duplicates_leave_every_list(fake, tmp_path):
    """A TANDUP whose first reads have a secondary twin in the same window: with the option the tables are those of the world
    without the twins."""
    base = synth.make_junction_world(5, ("TANDUP", "DEL"), ref_fraction=0.0)
    twins = synth.add_split_alignments(base, "hard", window_dups=3)
    assert twins.planted["window"] == 3
    text = synth.bed_text(base)
    out = {}
    for tag, w, more in (("twins_on", twins, ["--dedup-qname"]), ("twins_off", twins, []), ("base", base, [])):
        for extra in ([], ["--both-ends"]):
            seqio.set_backend(seqio.MemorySamtools(w))
            out[(tag, bool(extra))] = _main(tmp_path, tag + str(len(extra)), "bed", text, more + extra)[0]
    for be_on in (False, True):
        assert out[("twins_on", be_on)] == out[("base", be_on)] != out[("twins_off", be_on)]


def test_pack_and_unpack_carry_the_keys_and_leave_the_plain_record_alone():
    plain = [[0.5, -1.25], None, []]
    flat = bothends.pack(plain)
    assert flat == [3.0, 2.0, -1.0, 0.0, 0.5, -1.25] and bothends.unpack(flat) == plain
    assert getattr(bothends.unpack(flat), "keys", None) is None
    v = bothends.Views(plain)
    v.keys = [[(1 << 64) - 1, 0x0123456789ABCDEF], None, []]
    got = bothends.unpack(np.asarray(bothends.pack(v), dtype=np.float64))
    assert list(got) == plain and got.keys == v.keys
    assert bothends.pack(v)[:len(flat)] == flat
    assert bothends.pool(plain) == [0.5, -1.25] and bothends.pool([[1.0, 2.0], None, [3.0, 4.0]], [[7, 8], None, [8, 9]]) == [1.0, 2.0, 4.0]
    # a key twice in ONE view is not rule V's business
    assert bothends.pool([[1.0, 2.0], [3.0]], [[7, 7], [7]]) == [1.0, 2.0]

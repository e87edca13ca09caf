"""`--links` without a GPU: the SA grammar against the rule's regular expression applied here, the regions of
every row of the table of loci, links.answer against a brute force, the native host reader (vapor_bam_links) against both on
files written case by case, the three stand-alone programs under the sanitizers, the mode's surface, the refused combinations,
and cli.main on a world whose seven columns are known in closed form - in memory, through SAM text and from files on the host
routes."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import links_cases as LC
import readplan_program
import test_bamio as TB
import test_modes_cpu as TM
import test_signature_cpu as SC
from vapor_amd import _lib as L
from vapor_amd import bamio, cli, links, modes, pipeline, seqio, signature, synth

ROOT = SC.ROOT
BASE = SC.BASE
T, C, Q = LC.T, LC.C, LC.Q


# ------------------------------------------------------------------------------------------------------------------------------
# the parser
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_parser_takes_links_on_bed_and_vcf():
    assert cli.build_parser().parse_args(BASE).links is False
    assert cli.build_parser().parse_args(BASE + ["--links"]).links is True
    assert cli.build_parser().parse_args(BASE + ["--links", "--min-mapq", "20", "--exclude-flags", "0x800", "--dedup-qname", "--bnd", "--no-figures"]).links is True
    m = modes.LINKS
    assert m.name == "links" and m.chunk_payloads is not None and m.chunk_gens is None
    assert tuple(TM.hook_payloads(m)) == links.TYPES          # the hook answers for the module's types
    assert (links.C, links.T, links.TOL_MAX, links.EXCLUDE) == (30, 50, 255, 0x704) and links.EXCLUDE is signature.EXCLUDE
    assert links.events is signature.events                  # the clip events are not stated a second time


@pytest.mark.parametrize("cmd, more, message", [
    ("bed", ["--links", "--refine", "20"], "--links and --refine cannot be combined"),
    ("vcf", ["--links", "--phased"], "--links and --phased cannot be combined"),
    ("bed", ["--links", "--phase-vcf", "p.vcf"], "--links and --phase-vcf cannot be combined"),
    ("vcf", ["--links", "--both-ends"], "--links and --both-ends cannot be combined"),
    ("bed", ["--links", "--depth"], "--links and --depth cannot be combined"),
    ("vcf", ["--links", "--signatures"], "--links and --signatures cannot be combined"),
    ("svelter", ["--links"], "--links applies to `vapor bed` and `vapor vcf`"),
    ("ins", ["--links"], "--links applies to `vapor bed` and `vapor vcf`"),
])
def test_refused_option_combinations(cmd, more, message, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main([cmd] + BASE + more)
    assert e.value.code == 2 and message in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------------------------------------
# the SA grammar
# ------------------------------------------------------------------------------------------------------------------------------
def aux_value(aux):
    """bamio's reading of the SA value in an aux area that follows a 32-byte header without name, CIGAR and bases."""
    rec = struct.pack("<iiBBHHHiiii", 0, 0, 0, 0, 0, 0, 0, 0, -1, -1, 0) + aux
    return bamio.BamFile.sa_of_aux(rec, 32)


DESIGNED_VALUES = [
    (b"c,0,+,5M,60,0;", []), (b"c,2147483647,+,5M,60,0;", [(b"c", 2147483646, 2147483651, "+")]), (b"c,2147483648,+,5M,60,0;", []),
    (b"c,0000000100,-,5M,60,0;", [(b"c", 99, 104, "-")]), (b"c,00000000100,+,5M,60,0;", []),
    (b"c,100,+,268435455M,60,0;", [(b"c", 99, 99 + 268435455, "+")]), (b"c,100,+,268435456M,60,0;", []), (b"c,100,+,0000000005M,60,0;", []),
    (b"c,100,+,5M7,60,0;", []), (b"c,100,+,,60,0;", []), (b"c,100,+,*,60,0;", []), (b"c,100,.,5M,60,0;", []),
    (b"c,100,+,5M,256,0;", []), (b"c,100,+,5M,0060,0;", []), (b"c,100,+,5M,255,0;", [(b"c", 99, 104, "+")]),
    (b"c,100,+,5M,60,;", []), (b"c,100,+,5M,60,x;", []), (b"c,100,+,5M,60;", []), (b"c,100,+,5M,60,0,1;", []),
    (b"a,1,+,1M,0,0;;b,2,-,2D,0,0;", [(b"a", 0, 1, "+"), (b"b", 1, 3, "-")]), (b";;", []),
    (b"a,1,+,1M,0,0;b,2,-,3S2N1I,0,0", [(b"a", 0, 1, "+"), (b"b", 1, 3, "-")]), (b"", []), (None, []),
    (b"a,1,+,5M3I4D6N7S2H1P8=9X,0,77;", [(b"a", 0, 5 + 4 + 6 + 8 + 9, "+")]), (b"a b\t,1,+,1M,0,0", [(b"a b\t", 0, 1, "+")]),
]


def test_parse_sa_on_designed_values_and_aux_areas():
    for value, want in DESIGNED_VALUES:
        assert links.parse_sa(value) == want == LC.rule_entries(value), value
    # the cut on mapQ: an entry below it is ignored, one at it is not
    v = b"a,1,+,1M,19,0;b,1,+,1M,20,0;c,1,+,1M,255,0;"
    assert [e[0] for e in links.parse_sa(v, 20)] == [b"b", b"c"] and links.parse_sa(v, 20) == LC.rule_entries(v, 20) and len(links.parse_sa(v)) == 3
    for label, piece in LC.ILL_FORMED:
        assert links.parse_piece(LC.filled(piece)) is None and not LC.rule_entries(LC.filled(piece)), label
    for label, piece in LC.WELL_FORMED:
        assert links.parse_piece(LC.filled(piece))[:2] == (b"chr7", LC.Y) and LC.rule_entries(LC.filled(piece)), label
    # the aux area: the first field named SA decides; a type other than Z has no entries; damage before it leaves none
    good = b"SAZa,1,+,1M,0,0;\x00"
    assert aux_value(good) == b"a,1,+,1M,0,0;" and aux_value(b"NMC\x01" + good) == b"a,1,+,1M,0,0;"
    assert aux_value(b"SAAx" + good) is None and aux_value(b"SAH00\x00" + good) is None and aux_value(b"SAi\x01\x00\x00\x00" + good) is None
    assert aux_value(good + b"SAZb,1,+,1M,0,0;\x00") == b"a,1,+,1M,0,0;"
    assert aux_value(b"XYq\x01" + good) is None and aux_value(b"SAZa,1,+,1M,0,0;") is None and aux_value(b"") is None and aux_value(b"SA") is None
    assert aux_value(b"MLBC\x03\x00\x00\x00abc" + good) == b"a,1,+,1M,0,0;" and aux_value(b"MLBC\x09\x00\x00\x00abc" + good) is None
    assert aux_value(b"SAZ\x00") == b""
    assert links.sa_of_sam(["NM:i:3", "SA:Z:a,1,+,1M,0,0;", "SA:Z:b"]) == b"a,1,+,1M,0,0;" and links.sa_of_sam(["SA:A:x", "SA:Z:b"]) is None
    assert links.sa_of_sam([]) is None and links.sa_of_sam(["SA:Z:"]) == b""


def test_parse_sa_equals_the_regular_expression_on_seeded_bytes():
    rng = np.random.default_rng(5)
    alphabet = np.frombuffer(b"0123456789,;+-MIDNSHP=X*. abz", dtype=np.uint8)
    n_entries = 0
    for it in range(6000):
        pieces = []
        for _ in range(int(rng.integers(0, 4))):
            p = bytearray(LC.ent(bytes(rng.choice(alphabet[-3:], size=int(rng.integers(1, 5)))), int(rng.integers(0, 10 ** int(rng.integers(1, 11)))) - 1 + (rng.random() < 0.9), 0,
                                 (b"+", b"-")[int(rng.integers(0, 2))], mapq=int(rng.integers(0, 300)),
                                 cigar="".join("%d%s" % (int(rng.integers(0, 10 ** int(rng.integers(1, 10)))), "MIDNSHP=X"[int(rng.integers(0, 9))])
                                               for _ in range(int(rng.integers(1, 5))))) if rng.random() < 0.9 else b"x")
            for _ in range(int(rng.choice([0, 0, 1, 2]))):
                at = int(rng.integers(0, len(p)))
                how = int(rng.integers(0, 3))
                if how == 0:
                    p[at] = int(rng.choice(alphabet))
                elif how == 1:
                    p.insert(at, int(rng.choice(alphabet)))
                elif len(p) > 1:
                    del p[at]
            pieces.append(bytes(p))
        value = b";".join(pieces) + (b";" if rng.random() < 0.7 else b"")
        cut = int(rng.choice([0, 0, 20, 61]))
        got = links.parse_sa(value, cut)
        assert got == LC.rule_entries(value, cut), value
        n_entries += len(got)
    assert 1000 < n_entries < 12000, n_entries


# ------------------------------------------------------------------------------------------------------------------------------
# links.regions: every row of the table, at both ends of a contig
# ------------------------------------------------------------------------------------------------------------------------------
L_, R_ = links.LCLIP, links.RCLIP
A_, B_ = links.END_A, links.END_B
SAME, OTHER = links.SAME, links.OTHER


def test_regions_of_every_row_of_the_table():
    n = 100000
    length = {"c": n, "A": 5000, "B": 7000}.get
    s, e = 3001, 15000
    j0, j1 = 3000, 15000

    def reg(c, x, ev, pc, y, pend, rel, ln):
        return (c, (max(x - T - 1, 0), min(x + T + 1, ln), x, y, T, C, ev, pend, rel), pc)
    assert links.regions("DEL", ["c", s, e], length) == ([reg("c", j0, R_, "c", j1, A_, SAME, n)], [reg("c", j1, L_, "c", j0, B_, SAME, n)])
    assert links.regions("TANDUP", ["c", s, e], length) == ([reg("c", j0, L_, "c", j1, B_, SAME, n)], [reg("c", j1, R_, "c", j0, A_, SAME, n)])
    assert links.regions("INV", ["c", s, e], length) == ([reg("c", j0, R_, "c", j1, B_, OTHER, n), reg("c", j0, L_, "c", j1, A_, OTHER, n)],
                                                        [reg("c", j1, R_, "c", j0, B_, OTHER, n), reg("c", j1, L_, "c", j0, A_, OTHER, n)])
    p, q = 2000, 3000
    assert links.regions("BND", ["A", p, "B", q, "3to5", ""], length) == ([reg("A", p, R_, "B", q - 1, A_, SAME, 5000)], [reg("B", q - 1, L_, "A", p, B_, SAME, 7000)])
    assert links.regions("BND", ["A", p, "B", q, "3to3", "ACGT"], length) == ([reg("A", p, R_, "B", q, B_, OTHER, 5000)], [reg("B", q, R_, "A", p, B_, OTHER, 7000)])
    # a 5to3 record is scored at its mirrored 3to5 view (cli.bnd_view), a 5to5 record has no view without --both-ends
    view = cli.bnd_view("B", q, "]A:%d]T" % p)
    assert view[:5] == ["A", p, "B", q, "3to5"] and links.regions("BND", view, length) == links.regions("BND", ["A", p, "B", q, "3to5", ""], length)
    assert isinstance(cli.bnd_view("A", p, "[B:%d[T" % q), str)
    for t, locus in (("INS", ["c", 3000, 250]), ("DISDUP", ["c", s, e]), ("DEL_INV", ["c", s, e]), ("Other", ["c", s, e]), ("BND", ["A", p, "B", q, "5to5", ""]),
                     ("BND", ["A", p, "B"])):
        assert links.regions(t, locus, length) == ([], []) and links.payload(t, locus, [], []) is None


def test_regions_at_both_ends_of_a_contig():
    length = {"c": 4000, "A": 30, "B": 2000}.get
    # the event on the contig's first and last bases: J0 = 0, J1 = the contig's length; every window is clipped, none is refused
    left, right = links.regions("DEL", ["c", 1, 4000], length)
    assert left[0][1][:4] == (0, 51, 0, 4000) and right[0][1][:4] == (3949, 4000, 4000, 0)
    for side in links.regions("INV", ["c", 1, 4000], length) + links.regions("TANDUP", ["c", 20, 3990], length):
        for _c, f, pc in side:
            assert 0 <= f[0] <= f[1] <= 4000 and links.region_ok(f, pc)
    # a breakend at the last base of A and the first of B; a locus behind the contig's end has empty windows
    left, right = links.regions("BND", ["A", 30, "B", 1, "3to5", ""], length)
    assert left[0][1][:4] == (0, 30, 30, 0) and right[0][1][:4] == (0, 51, 0, 30)
    left, right = links.regions("DEL", ["c", 9001, 9500], length)
    assert left[0][1][:2] == (4000, 4000) and right[0][1][:2] == (4000, 4000)
    left, right = links.regions("DEL", ["nowhere", 100, 900], lambda c: 0)
    assert left[0][1][:2] == (0, 0) and right[0][1][:2] == (0, 0)


# ------------------------------------------------------------------------------------------------------------------------------
# links.answer against the brute force
# ------------------------------------------------------------------------------------------------------------------------------
def as_records(recs, flt=(0, 0)):
    """brute's dicts as links.answer takes them, the filter applied."""
    return [(r["pos0"] + 1, signature.parse_cigar(r["cigar"]), r["flag"], r["sa"]) for r in recs
            if r["mapq"] >= flt[0] and not r["flag"] & (flt[1] | LC.EXCLUDE)]


def test_answer_equals_the_brute_force_on_seeded_and_designed_records():
    rows, recs, cases = LC.seeded_world(np.random.default_rng(8), 1500, 200)
    seen = [0, 0, 0]
    for flt in ((0, 0), (Q, 0x800)):
        given = as_records(recs, flt)
        for _name, _c, f, partner, _e, _s in cases:
            got = links.words(links.answer(given, f, partner, flt[0]))
            assert got == LC.brute(recs, f, partner, flt), (f, partner, flt)
            seen = [a + (b > 0) for a, b in zip(seen, got)]
    assert min(seen) > 40, seen
    d = LC.designed_cases()
    for name, chrom, f, partner, expect, _status in d.cases:
        recs = d.recs[{"c": 0, "d": 1}[chrom]]
        got = links.words(links.answer(as_records(recs), f, partner))
        assert got == LC.brute(recs, f, partner) and (expect is None or got == expect), (name, got, expect)
    # what is refused: the one statement of the readers
    good = (100, 300, 200, 200, 50, 30, 0, 0, 0)
    assert links.region_ok(good, b"c")
    for k, v in ((0, -1), (0, 301), (1, 1 << 31), (4, -1), (4, 256), (6, 2), (6, -1), (7, 2), (8, 2)):
        bad = list(good)
        bad[k] = v
        assert not links.region_ok(bad, b"c"), (k, v)
        with pytest.raises(ValueError):
            links.answer([], bad, b"c")
    assert not links.region_ok(good, b"")


def test_merge_and_payload_and_columns():
    assert links.merge_words([1, 2, 3, 4, 2], [5, 1, 1, -4, 2]) == [6, 3, 4, -4, 2]
    assert links.merge_words([0] * 5, [1, 1, 1, 7, 1]) == [1, 1, 1, 7, 1] and links.merge_words([3, 2, 0, 0, 0], [1, 0, 0, 0, 0]) == [4, 2, 0, 0, 0]
    # an INV side: the counts of its two regions summed, of their modes the better kept
    p = links.payload("INV", ["c", 3001, 15000], [[5, 4, 3, 2, 2], [4, 4, 4, -1, 3]], [[9, 9, 2, 5, 1], [1, 1, 1, -5, 1]])
    assert list(p) == [7, 8, 3, 10, -1, 3, -5, 1] and (p.start, p.end) == (3001, 15000)
    assert links.columns(p) == ["7", "3", "7", "1", "7", str(3001 - 5), str(15000 - 1)]
    p = links.payload("BND", ["A", 2000, "B", 3000, "3to5", ""], [[4, 3, 3, 1, 3]], [[2, 0, 0, 0, 0]])
    assert links.columns(p) == ["3", "0", "3", "0", "0", ".", "3001"] and (p.start, p.end) == (2000, 3000)


# ------------------------------------------------------------------------------------------------------------------------------
# the native host reader on files written case by case
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def designed(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("links") / "designed.bam")
    return path, LC.write_designed(path, 1000)


@pytest.fixture(scope="module")
def seeded(tmp_path_factory):
    rows, recs, cases = LC.seeded_world(np.random.default_rng(12))
    path = str(tmp_path_factory.mktemp("links_seeded") / "seeded.bam")
    bamio.write_bam(path, [("c", 60000)], rows, block_size=20000)
    return path, recs, cases


def python_statement(path, chrom, f, partner, flt=(0, 0)):
    b = bamio.BamFile(path)
    b.set_filter(*flt)
    recs = b.fetch_links(chrom, f[0] + 1, f[1], exclude_more=links.EXCLUDE) if f[1] > f[0] else []
    return links.words(links.answer(recs, f, partner, flt[0]))


@pytest.mark.parametrize("flt", [(0, 0), (0, 0x800), (Q, 0), (Q, 0x810)])
def test_native_reader_equals_the_statement_and_the_brute_force(designed, seeded, flt, monkeypatch):
    monkeypatch.setenv("VAPOR_BAM_DEVICE", "0")
    for path, by_tid, cases in ((designed[0], designed[1].recs, designed[1].cases), (seeded[0], {0: seeded[1]}, seeded[2][:120])):
        be = seqio.InProcessBam()
        be.read_filter = flt
        chroms = [c[1] for c in cases] + ["nowhere"]
        regions = [c[2] for c in cases] + [(0, 30, 10, 20, 5, C, 0, 0, 0)]
        partners = [c[3] for c in cases] + [b"c"]
        got = be.links_many(None, path, chroms, regions, partners)
        assert got[-1] == [0] * 5
        for (name, chrom, f, partner, expect, _s), g in zip(cases, got):
            want = LC.brute(by_tid[{"c": 0, "d": 1}[chrom]], f, partner, flt)
            assert g == want, (name, g, want)
            if flt == (0, 0) and expect is not None:
                assert g == expect, (name, g, expect)
        for k in range(0, len(cases), 7):
            assert got[k] == python_statement(path, chroms[k], regions[k], partners[k], flt)
        # the Python route of links_many (VAPOR_BAM_NATIVE=0, or a library without the entries) gives the same
        monkeypatch.setenv("VAPOR_BAM_NATIVE", "0")
        assert be.links_many(None, path, chroms, regions, partners) == got
        monkeypatch.delenv("VAPOR_BAM_NATIVE")
    by_name = {c[0]: k for k, c in enumerate(designed[1].cases)}
    be = seqio.InProcessBam()
    be.read_filter = flt
    c = designed[1].cases[by_name["an entry below the cut"]]
    assert be.links_many(None, designed[0], [c[1]], [c[2]], [c[3]])[0] == ([2, 2, 2, 0, 1] if flt[0] == 0 else [2, 1, 1, 4, 1])
    c = designed[1].cases[by_name["records that never count, and the user's filter"]]
    assert be.links_many(None, designed[0], [c[1]], [c[2]], [c[3]])[0][0] == {(0, 0): 5, (0, 0x800): 4, (Q, 0): 4, (Q, 0x810): 2}[flt]

    class Without:
        def __getattr__(self, name):
            if name in ("vapor_bam_links", "vapor_bam_links_device"):
                raise AttributeError(name)
            return getattr(L.load(), name)
    real = L.load()
    monkeypatch.setattr(L, "_lib", Without())
    called = []
    monkeypatch.setattr(bamio.BamFile, "links_native", lambda self, *a, **k: called.append(a))
    cases = designed[1].cases[:40]
    got = seqio.InProcessBam.links_many(be, None, designed[0], [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases])
    assert not called and got == [LC.brute(designed[1].recs[0], c[2], c[3], flt) for c in cases]
    monkeypatch.setattr(L, "_lib", real)


def test_dedup_has_no_effect_and_fetch_raw_is_what_it_was(designed):
    path, d = designed
    b = bamio.BamFile(path)
    name, chrom, f, partner, expect, _s = d.cases[0]
    row = list(f) + [0, len(partner)]
    want = b.links_native(0, row, None, partner)
    b.set_dedup(True)
    assert b.links_native(0, row, None, partner) == want == expect
    raw = b.fetch_raw(chrom, f[0] + 1, f[1])
    assert raw and all(len(r) == 7 for r in raw)             # (QNAME, POS, operations, SEQ, l_seq, FLAG, tags): no eighth field
    got = b.fetch_links(chrom, f[0] + 1, f[1])
    assert [(r[1], r[5]) for r in raw] == [(g[0], g[2]) for g in got] and got[0][3] == LC.ent(LC.P, LC.Y) + b";"
    b.close()


def test_native_reader_refuses_bad_regions(designed):
    path, _ = designed
    b = bamio.BamFile(path)
    ch = [(b.first_record, b.first_record + 1)]
    good = (100, 300, 200, 200, 50, 30, 0, 0, 0, 1, 2)
    assert b.links_native(0, good, ch, b"abc") == [0] * 5
    for k, v in ((0, -1), (0, 301), (1, 1 << 31), (4, -1), (4, 256), (6, 2), (6, -1), (7, 2), (8, -1), (10, 0), (10, 3), (9, -1), (9, 4)):
        bad = list(good)
        bad[k] = v
        with pytest.raises(ValueError, match="vapor_bam_links"):
            b.links_native(0, bad, ch, b"abc")
    with pytest.raises(ValueError):
        b.links_native(-1, good, ch, b"abc")
    with pytest.raises(ValueError):
        b.links_native(0, good, ch, b"")
    b.close()


def test_abi_surface():
    h = open(os.path.join(ROOT, "include", "vapor_hip.h")).read()
    for name in ("vapor_bam_links", "vapor_bam_links_device"):
        assert re.search(r"\bint %s\(" % name, h) and name in L.EXPORTS and name in L.OPTIONAL_EXPORTS and hasattr(L.load(), name)
    assert L.ABI_VERSION == 3
    from vapor_amd import build
    assert os.path.join(build.CSRC, "vapor_sa.h") in build.DEPS and os.path.join(build.CSRC, "vapor_sa.h") not in build.KERNEL_FILES
    sa = open(os.path.join(build.CSRC, "vapor_sa.h")).read()
    assert "hip" not in sa.replace("HIP-free", "").lower()


# ------------------------------------------------------------------------------------------------------------------------------
# the stand-alone programs under the sanitizers
# ------------------------------------------------------------------------------------------------------------------------------
SAN = SC.SAN


def test_the_sa_grammar_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sa_check")
    r = subprocess.run(["g++", "-std=c++17"] + SAN + [os.path.join(ROOT, "tools", "sa_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert lines[-1] == "sa_check: all equal" and len(lines) == 5
    assert int(re.search(r"\((\d+) well-formed\)", lines[1]).group(1)) > 2000


def test_links_pass_under_sanitizers_on_good_and_damaged_files(designed, tmp_path):
    exe = str(tmp_path / "bam_check")
    r = subprocess.run(["g++", "-std=c++17"] + SAN + ["-o", exe, os.path.join(ROOT, "tools", "bam_check.cpp"), "-lz", "-lpthread"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(path, first, win, *more):
        p = subprocess.run([exe, path, str(first), "0", str(win[0]), str(win[1]), "200", "2"] + [str(m) for m in more], env=env,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, (path, p.returncode, p.stderr[-2000:])
        return p.stdout.splitlines()
    # a file of its own whose records name the tool's partner "c1": every record of the file walked, eight regions a contig
    x, y = 5000, 9000
    rows, recs = [], []
    rng = np.random.default_rng(3)
    for i in range(300):
        ev = int(rng.integers(0, 2))
        name = (b"c1", b"c1", b"c", b"c10", b"c0")[int(rng.integers(0, 5))]
        value = LC.ent(name, y + int(rng.integers(-60, 61)), int(rng.integers(0, 2)), (b"+", b"-")[int(rng.integers(0, 2))], mapq=int(rng.choice([5, 60]))) + b";"
        if i % 9 == 0:
            value = LC.filled(LC.ILL_FORMED[i % len(LC.ILL_FORMED)][1]) + b";" + value
        at = x + int(rng.integers(-60, 61))
        cigar = "100M40S" if ev else "40S100M"
        pos0 = at - 100 if ev else at
        flag, mapq = int(rng.choice([0, 0x10, 0x800, 0x400])), int(rng.choice([60, 19]))
        before = (b"", b"NMC\x01", b"XYq\x00" if i % 50 == 7 else b"")[i % 3]
        rows.append(("r%d" % i, 0, pos0, cigar, "A" * 140, before + b"SAZ" + value + b"\x00", mapq, flag))
        recs.append(dict(pos0=pos0, cigar=cigar, flag=flag, mapq=mapq, sa=None if before[:2] == b"XY" else value))
    path = str(tmp_path / "tool.bam")
    bamio.write_bam(path, [("c", 20000), ("e", 1000)], rows, block_size=3000)
    first = bamio.BamFile(path).first_record
    for flt in ((), (Q, 0x800)):
        out = [ln for ln in run(path, first, (x, y), *flt, "links") if ln.startswith("links:")]
        assert len(out) == 16
        total = 0
        for ln in out[:8]:
            f = ln.split()
            ev, pend, rel = int(f[4]), int(f[6]), int(f[8])
            want = LC.brute(recs, (0, (1 << 31) - 1, x, y, 50, 30, ev, pend, rel), b"c1", flt or (0, 0))
            assert f[:3] == ["links:", "contig", "0"] and f[9:11] == ["rc", "0"] and [int(v) for v in f[12:17]] == want, ln
            total += want[2]
        assert total > 5 and all(ln.split()[12:17] == ["0"] * 5 for ln in out[8:])
    assert not any(ln.startswith("links:") for ln in run(path, first, (x, y)))
    # the damaged files of tests/test_bamio.py: a status, never a report
    small = TB._small_bam(tmp_path)
    first = bamio.BamFile(small).first_record
    assert run(small, first, (4000, 5500), "links")[-1].startswith("links: contig 1 ev 1 pend 1 rel 1 rc 0 words ")
    raw = open(small, "rb").read()
    off, bsize, xlen = TB._blocks(raw)[6]
    n_err = 0
    for field in ("isize_huge", "isize_small", "bsize_tiny", "bsize_big", "crc", "payload_bit", "xlen_big", "truncated"):
        b = bytearray(raw)
        if field == "isize_huge":
            struct.pack_into("<I", b, off + bsize - 4, 0xFFFFFFFF)
        elif field == "isize_small":
            struct.pack_into("<I", b, off + bsize - 4, 17)
        elif field == "bsize_tiny":
            struct.pack_into("<H", b, off + 16, 9)
        elif field == "bsize_big":
            struct.pack_into("<H", b, off + 16, 0xFFFF)
        elif field == "crc":
            b[off + bsize - 8] ^= 0x40
        elif field == "payload_bit":
            b[off + 12 + xlen + (bsize - xlen - 20) // 2] ^= 0x04
        elif field == "xlen_big":
            struct.pack_into("<H", b, off + 10, 0xFFF0)
        else:
            b = b[:off + bsize // 2]
        bad = str(tmp_path / ("v_%s.bam" % field))
        open(bad, "wb").write(bytes(b))
        lines = [ln for ln in run(bad, first, (4000, 5500), "links") if ln.startswith("links: contig 0 ev 0 pend 0 rel 0 rc ")]
        assert len(lines) == 1, lines
        n_err += lines[0].startswith("links: contig 0 ev 0 pend 0 rel 0 rc -4")
    assert n_err >= 7, n_err              # (a file cut between two blocks may end like one without EOF marker)
    # the designed file, whose aux areas are damaged on purpose in two records: the pass ends in words, not in a report
    d_first = bamio.BamFile(designed[0]).first_record
    assert len([ln for ln in run(designed[0], d_first, (5000, 9000), "links") if " rc 0 " in ln and ln.startswith("links:")]) == 16


def test_the_plan_of_the_device_call_under_sanitizers():
    lines = readplan_program.output().splitlines()
    assert lines[-1] == "readplan_check: all equal"
    lk = [ln for ln in lines if ln.startswith("links plan: ")]
    assert len(lk) == 1 and "the name blob, clamped fields and collected words equal the rule" in lk[0] and 'both size refusals say "in one call"' in lk[0]
    assert int(lk[0].split()[2]) == 1000 and int(re.search(r"\((\d+) refused\)", lk[0]).group(1)) > 1000


# ------------------------------------------------------------------------------------------------------------------------------
# the mode's surface
# ------------------------------------------------------------------------------------------------------------------------------
def test_payload_round_trip_and_columns():
    m = modes.LINKS
    assert m.pack(None) == [] and m.unpack(m.pack(None)) is None and m.unpack([]) is None
    for x in (links.Payload([4, 6, 5, 6, -3, 4, 7, 5], 3001, 15000), links.Payload([0] * 8, 1, 300),
              links.Payload([(1 << 32) - 1, (1 << 32) - 1, 1, 2, -255, 1, 255, 1], (1 << 31) - 60, (1 << 31) - 1)):
        flat = m.pack(x)
        assert flat and all(isinstance(v, float) for v in flat)
        back = m.unpack(flat)
        assert type(back) is links.Payload and list(back) == list(x) and (back.start, back.end) == (x.start, x.end)
        assert len(m.columns_many([x, None])[0]) == len(m.COLUMNS)
    assert len(m.COLUMNS) == len(m.INFO) == len(m.keys) == len(m.columns_many([None])[0]) == 7
    assert m.columns_many([None])[0] == ["."] * 7
    assert list(m.COLUMNS) == ["VaPoR_LNK_L", "VaPoR_LNK_R", "VaPoR_LNK_N", "VaPoR_LNK_OL", "VaPoR_LNK_OR", "VaPoR_LNK_POS", "VaPoR_LNK_END"]
    assert all(len(i) == 4 and i[1] == "Integer" and i[3].endswith("(--links)") for i in m.INFO)
    assert m.attr == "links" and tuple(m.keys) == tuple(m.COLUMNS) and m.skip_dot and not m.phased
    # N = max(L, R); OL, OR = n_split - n_link; POS = start + the right side's offset, END = end + the left side's; '.' without a mode
    assert m.columns_many([links.Payload([4, 6, 5, 6, -3, 4, 7, 5], 3001, 15000)]) == [["4", "5", "5", "2", "1", "3008", "14997"]]
    assert m.columns_many([links.Payload([0, 3, 2, 2, 0, 0, 0, 2], 3001, 3300)]) == [["0", "2", "2", "3", "0", "3001", "."]]
    assert m.columns_many([links.Payload([0] * 8, 3001, 3300)]) == [["0", "0", "0", "0", "0", ".", "."]]


# ------------------------------------------------------------------------------------------------------------------------------
# cli.main on a world whose columns are known
# ------------------------------------------------------------------------------------------------------------------------------
fake = SC.fake
READS = 4
JITTER = (0, 3, 0, -2)


def closed_form(w, reads=READS, jitter=JITTER, min_mapq=0, exclude=0):
    """The seven columns of every locus of make_links_world from its parameters.  Each junction has `reads` molecules, a linked
    record on each side; an INV has two junctions, and a side's regions see one each.  The decoys: two split records at the
    left breakpoint whose entries lie elsewhere (OL = 2), one at the right on the wrong strand (OR = 1), and at the right a good
    entry of mapQ 3 - a link at offset 0 unless --min-mapq cuts it, in which case the record has no entry left.  The offsets:
    molecule k reports the first coordinate jitter[k] to the right, and the second with it - by the same amount when the two
    events differ (DEL, TANDUP, 3to5), by the opposite when they are the same (INV, 3to3).  POS is read from the right side
    (whose partner is the first coordinate), END from the left.  With 0x800 excluded a molecule's supplementary record - the one
    at its second coordinate - is gone, and with it the right side's links."""
    out = []
    for l in w.loci:
        form = (l.extra or {}).get("form", l.svtype)
        n = reads * (2 if l.svtype == "INV" else 1)
        first = [jitter[k % len(jitter)] for k in range(reads)]
        second = first if form in ("DEL", "TANDUP", "3to5") else [-d for d in first]
        low = min_mapq <= synth.LINKS_DECOY_MAPQ
        right_links = ([] if exclude & 0x800 else first) + ([0] if low else [])
        right_n = (0 if exclude & 0x800 else n) + (1 if low else 0)

        def mode(offs):
            return sorted(set(offs), key=lambda o: (-offs.count(o), abs(o), o))[0] if offs else None
        pos, end = mode(right_links), mode(second)
        out.append([str(n), str(right_n), str(max(n, right_n)), "2", "1", "." if pos is None else str(l.start + pos), str(l.end + end)])
    return out


def test_closed_form_of_the_world_by_hand():
    w = synth.make_links_world(seed=4, reads=READS, jitter=JITTER)
    cf = closed_form(w)
    # jitter (0, 3, 0, -2): the first coordinate's mode is 0 (two of four, three with the low-mapQ decoy), the second's too
    assert [(l.svtype, (l.extra or {}).get("form")) for l in w.loci] == [("DEL", None), ("TANDUP", None), ("INV", None), ("BND", "3to5"), ("BND", "3to3")]
    assert cf[0] == ["4", "5", "5", "2", "1", "3001", "15000"] and cf[2] == ["8", "9", "9", "2", "1", "3001", "15000"]
    assert cf[3] == ["4", "5", "5", "2", "1", "3000", "3000"] == cf[4]
    assert closed_form(w, min_mapq=5)[0] == ["4", "4", "4", "2", "1", "3001", "15000"]
    # jitter (2, 2, 0, -1) with the decoy cut: the mode is 2 - on the second coordinate of an INV that is 2 to the left
    assert closed_form(w, jitter=(2, 2, 0, -1), min_mapq=5)[2][-2:] == ["3003", "14998"] and closed_form(w, jitter=(2, 2, 0, -1), min_mapq=5)[0][-2:] == ["3003", "15002"]
    # ... and with the decoy's link at offset 0 the first coordinate ties at two each: the smaller offset wins
    assert closed_form(w, jitter=(2, 2, 0, -1))[0][-2:] == ["3001", "15002"]
    flags = {r.flag for rs in w.reads.values() for r in rs}
    assert {0, 0x10, 0x800, 0x810} <= flags
    # every alt read is a primary and a supplementary record that name each other
    by_q = {}
    for c, rs in w.reads.items():
        for r in rs:
            assert sum(o >> 4 for o in signature.parse_cigar(r.cigar) if o & 15 in (0, 1, 4, 7, 8)) == len(r.seq), r.qname
            if re.search(r"_m\d+$", r.qname):
                by_q.setdefault(r.qname, []).append(r)
    assert len(by_q) == READS * 6
    for q, (r1, r2) in by_q.items():
        assert sorted((r1.flag & 0x800, r2.flag & 0x800)) == [0, 0x800]
        for me, you in ((r1, r2), (r2, r1)):
            (name, a, b, strand), = links.parse_sa(me.tags["SA"].encode())
            assert (name.decode(), a + 1, "-" if you.flag & 0x10 else "+") == (you.rname, you.pos, strand) and b - a == signature.parse_cigar(you.cigar)[0 if you.cigar.endswith("S") else 1] >> 4
    # the existing worlds and add_split_alignments are what they were: no record of theirs carries an SA tag
    old = synth.add_split_alignments(synth.make_junction_world(seed=3, n_reads=4))
    assert not any(r.tags and "SA" in r.tags for rs in old.reads.values() for r in rs)


def columns_of(table):
    rows = [r.split("\t") for r in table.splitlines()]
    assert rows[0][-7:] == list(links.COLUMNS)
    return rows


def test_cli_on_a_links_world_in_memory_and_through_sam_text(fake, tmp_path):
    w = synth.make_links_world(seed=4, reads=READS, jitter=JITTER)
    expect = closed_form(w)
    text = synth.bed_text(w)
    seqio.set_backend(seqio.MemorySamtools(w))
    plain, _ = SC.run_main(tmp_path, "plain", "bed", text)
    seqio.set_backend(seqio.MemorySamtools(w))
    table, _ = SC.run_main(tmp_path, "lnk", "bed", text, ["--links"])
    rows = columns_of(table)
    assert "\n".join("\t".join(r[:-7]) for r in rows) + "\n" == plain and "VaPoR_LNK" not in plain
    simple = [l for l in w.loci if l.svtype != "BND"]
    assert len(rows) == len(simple) + 1
    for r, l, e in zip(rows[1:], w.loci, expect):
        assert r[-7:] == e, (l, r[-7:], e)
    # --dedup-qname has no effect; --min-mapq cuts the entry of mapQ 3; 0x800 takes the supplementary records
    for more, kw in ((["--dedup-qname"], {}), (["--min-mapq", "5"], {"min_mapq": 5}), (["--exclude-flags", "0x800"], {"exclude": 0x800})):
        seqio.set_backend(seqio.MemorySamtools(w))
        t2, _ = SC.run_main(tmp_path, "more" + more[0], "bed", text, ["--links"] + more)
        assert [r[-7:] for r in columns_of(t2)[1:]] == closed_form(w, **kw)[:len(simple)], more
    # vcf --bnd: DEL and INV records and both breakends get the INFO keys; TANDUP is not scored by `vapor vcf`
    vtext = synth.links_vcf_text(w)
    seqio.set_backend(seqio.MemorySamtools(w))
    vplain, _ = SC.run_main(tmp_path, "vplain", "vcf", vtext, ["--bnd"])
    seqio.set_backend(seqio.MemorySamtools(w))
    vtable, annotated = SC.run_main(tmp_path, "vlnk", "vcf", vtext, ["--bnd", "--links"])
    vrows = columns_of(vtable)
    assert "\n".join("\t".join(r[:-7]) for r in vrows) + "\n" == vplain
    by_chrom = {r[0].split(":")[0]: r[-7:] for r in vrows[1:]}
    assert len(by_chrom) == 4
    for l, e in zip(w.loci, expect):
        if l.svtype != "TANDUP":
            assert by_chrom[l.chrom] == e, l
    lines = annotated.splitlines()
    assert sum(ln.startswith("##INFO=<ID=VaPoR_LNK_") for ln in lines) == 7
    rec = {ln.split("\t")[2]: ln.split("\t")[7] for ln in lines if not ln.startswith("#")}
    assert rec["lk1"].endswith(";VaPoR_LNK_L=4;VaPoR_LNK_R=5;VaPoR_LNK_N=5;VaPoR_LNK_OL=2;VaPoR_LNK_OR=1;VaPoR_LNK_POS=3001;VaPoR_LNK_END=15000")
    assert rec["lk4_1"].endswith(";VaPoR_LNK_POS=3000;VaPoR_LNK_END=3000") and rec["lk4_2"].endswith(";VaPoR_LNK_POS=3000;VaPoR_LNK_END=3000")
    assert set(rec) == {"lk1", "lk3", "lk4_1", "lk4_2", "lk5_1", "lk5_2"} and all("VaPoR_LNK_N=" in v for v in rec.values())
    # without --bnd the breakend rows are not scored, and the others' columns stay
    seqio.set_backend(seqio.MemorySamtools(w))
    nobnd, _ = SC.run_main(tmp_path, "nobnd", "vcf", synth.vcf_text(synth_without_bnd(w)), ["--links"])
    assert [r[-7:] for r in columns_of(nobnd)[1:]] == [expect[0], expect[2]]
    # the SAM text backends read the optional fields of the lines: the same five words per region
    mem = seqio.MemorySamtools(w)

    class Text(seqio.SamtoolsCLI):
        def __init__(self):
            self.read_filter = (0, 0)

        def view_lines(self, bam, region):
            return mem.view_lines(bam, region)

        def fai_lines(self, ref):
            return mem.fai_lines(ref)
    txt = Text()
    for flt in ((0, 0), (5, 0x800)):
        txt.read_filter = mem.read_filter = flt
        for l in w.loci:
            locus = [l.chrom, l.start, l.extra["mate_chrom"], l.end, l.extra["form"], ""] if l.svtype == "BND" else [l.chrom, l.start, l.end]
            left, right = links.regions(l.svtype, locus, lambda c: txt.contig_length("x", "r", c))
            regs = left + right
            args = ([r[0] for r in regs], [r[1] for r in regs], [r[2] for r in regs])
            got = txt.links_many(None, "x", *args)
            assert got == mem.links_many(None, "x", *args) and len(got) == len(regs) and (flt != (0, 0) or got[0][2] == READS)
    assert issubclass(seqio.SamtoolsHybrid, seqio.SamtoolsCLI) and seqio.SamtoolsHybrid.links_many is seqio.SamtoolsCLI.links_many


def synth_without_bnd(w):
    s = synth.SynthWorld()
    s.loci = [l for l in w.loci if l.svtype != "BND"]
    return s


def test_cli_from_files_on_the_host_routes(fake, tmp_path, monkeypatch):
    """The native host reader and the Python statement (VAPOR_BAM_NATIVE=0) from files, and the world in memory: byte-identical
    tables, the closed form's columns."""
    w = synth.make_links_world(seed=9, reads=READS, jitter=JITTER)
    expect = closed_form(w)
    fa, bam = synth.write_world_files(w, str(tmp_path), block_size=4096)
    vtext = synth.links_vcf_text(w)
    more = ["--bnd", "--links", "--min-mapq", "2"]
    monkeypatch.setenv("VAPOR_BAM_DEVICE", "0")
    seqio.set_backend(None)
    host, _ = SC.run_main(tmp_path, "host", "vcf", vtext, more, fa, bam)
    monkeypatch.setenv("VAPOR_BAM_NATIVE", "0")
    seqio.set_backend(None)
    py, _ = SC.run_main(tmp_path, "py", "vcf", vtext, more, fa, bam)
    monkeypatch.delenv("VAPOR_BAM_NATIVE")
    seqio.set_backend(seqio.MemorySamtools(w))
    mem, _ = SC.run_main(tmp_path, "mem", "vcf", vtext, more)
    assert host == py == mem
    by_chrom = {r[0].split(":")[0]: r[-7:] for r in columns_of(host)[1:]}
    assert len(by_chrom) == 4
    for l, e in zip(w.loci, expect):
        if l.svtype != "TANDUP":
            assert by_chrom[l.chrom] == e, l

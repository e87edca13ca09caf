"""`--realign-polish` without a device: the numpy statement (polish.statement) against the plain-integer model
(tests/polish_model.py) on every designed locus and a seeded fuzz, the model's nine mutants every one of which those loci tell
from the rule at least three times, `apply` against a text built by hand, the columns and their round trip, the parser, the
header's prototype and the export lists, the host plan of the call under the sanitizers as a program of its own
(tools/polish_check.cpp), and cli.main on an engine whose `realign`, `realign_trace` and `realign_polish` are the statements."""
import os
import re
import subprocess

import numpy as np
import pytest

import polish_model as M
import test_realign_cpu as TR
import test_signature_cpu as TS
import test_trace_cpu as TT
from conftest import ROOT
from vapor_amd import _lib as L
from vapor_amd import cli, modes, pipeline, polish, realign, seqio, synth


# ------------------------------------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------------------------------------
def stated(pairs, allele, band):
    """polish.statement in the model's shape."""
    counts, calls, sites, ins, stats = polish.statement([(r.decode("latin-1"), o) for r, o in pairs], allele.decode("latin-1"), band)
    k = int(stats[polish.SITES])
    assert not sites[k:].any() and not ins[k:].any()
    return (counts.tolist(), calls.tolist(), sites[:k].tolist(), [bytes(ins[s][:sites[s][1]]) for s in range(k)], stats.tolist()), (calls, sites, ins)


def test_the_constants_are_the_models_and_the_headers():
    assert (polish.MIN_COV, polish.RMAX, polish.MAX_SITES) == (M.MIN_COV, M.RMAX, M.MAX_SITES) == (3, 64, 256)
    assert (polish.KEEP, polish.DELETE, polish.SITE_BIT) == (M.KEEP, M.DELETE, M.SITE_BIT) == (4, 5, 8)
    h = open(os.path.join(ROOT, "vapor_amd", "csrc", "vapor_polish_plan.h")).read()
    for name, v in (("MIN_COV", 3), ("RMAX", 64), ("MAX_SITES", 256)):
        assert re.search(r"constexpr int %s = %d;" % (name, v), h), name
    assert "CALL_KEEP = 4, CALL_DELETE = 5, SITE_BIT = 8" in h


def test_the_statement_equals_the_model_on_every_designed_locus():
    loci, expect = M.designed_loci(), M.designed_expected()
    assert len(loci) >= 80
    wrong = []
    for (name, pairs, allele, band), e in zip(loci, expect):
        got, (calls, sites, ins) = stated(pairs, allele, band)
        if got != tuple(e):
            wrong.append((name, got[4], e[4]))
        assert polish.apply(allele.decode("latin-1"), calls, sites, ins) == M.text(allele, *e[1:4]).decode("latin-1"), name
    assert not wrong, (len(wrong), wrong[:3])


def test_the_statement_equals_the_model_on_the_fuzz():
    for name, pairs, allele, band in M.fuzz_loci():
        assert stated(pairs, allele, band)[0] == tuple(M.polish(pairs, allele, band)), name


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_mutant_is_told_from_the_rule_by_three_designed_loci(mutant):
    assert len(M.MUTANTS) == 9
    assert M.told_apart(mutant) >= 3, (mutant, M.told_apart(mutant))


def test_the_designed_loci_the_section_names_are_there():
    by = dict(zip((l[0] for l in M.designed_loci()), M.designed_expected()))
    # MIN_COV: nothing is called below three reads; the planted substitution, deletion and insertion from three on
    for k in (0, 1, 2):
        assert by["%d identical planted reads" % k][4] == [0, k, 0, 0, 0, 0, 0, 0]
    for k in (3, 4, 5):
        s = by["%d identical planted reads" % k][4]
        assert s[:5] == [0, k, 150, 1, 1] and s[6] == 3 and s[7] == 0
    # the strict majority: 2 of 4 keeps, 3 of 5 calls
    assert by["2 planted of 4"][4] == [0, 4, 150, 0, 0, 0, 0, 0] and by["3 planted of 5"][4][3:7:3] == [1, 3]
    # insertions at the edge of a read's coverage are none
    assert by["insertion before the first covered column"][4][5:] == [0, 0, 0]
    assert by["insertion behind the last covered column"][4][5:] == [0, 0, 0]
    # an allele N under a base majority is substituted; a read N never wins; lower case is kept
    assert by["allele N, 3 reads"][4][3] == 3 and by["allele N, 2 reads"][4][3] == 0
    assert by["read N, 4 reads of 5"][4][3:5] == [0, 0]
    loci = {l[0]: l for l in M.designed_loci()}
    l = loci["lower-case allele, 3 planted reads"]
    out = M.text(l[2], *by[l[0]][1:4])
    assert any(c in b"acgt" for c in out) and out != l[2]
    # inserted stretches of 1, 63, 64 and 65 bases: at most RMAX are kept
    for n_ins, want in ((1, 1), (63, 63), (64, 64), (65, 64)):
        for band in (100, 256):
            e = by["insertion of %d B=%d" % (n_ins, band)]
            assert e[4][6] >= want - 3 and max(s[1] for s in e[2]) <= M.RMAX, (n_ins, band, e[4])
    # the tie to the smallest code, and the majority of inserting reads at once
    assert by["two A and two C of five"][3] == [b"A"] == by["two C and two A of five"][3]
    # more than MAX_SITES sites: the model itself counts them
    s = by["more than 256 sites"][4]
    assert s[5] == M.MAX_SITES and s[7] > 0 and s[5] + s[7] > 256 and s[6] == 256


def test_apply_against_a_text_built_by_hand():
    allele = "acgtNACGTacgt"
    calls = np.full(len(allele), polish.KEEP, dtype=np.uint8)
    calls[1] = 3                                     # c -> T
    calls[4] = 0 | polish.SITE_BIT                   # GG before the N, the N -> A
    calls[6] = polish.DELETE
    calls[9] = polish.KEEP | polish.SITE_BIT         # an empty site
    calls[12] = polish.DELETE | polish.SITE_BIT      # C before the last column, which goes
    sites = np.zeros((polish.MAX_SITES, 2), dtype=np.int32)
    sites[:3] = [(4, 2), (9, 0), (12, 1)]
    ins = np.zeros((polish.MAX_SITES, polish.RMAX), dtype=np.uint8)
    ins[0, :2] = (ord("G"), ord("G"))
    ins[2, 0] = ord("C")
    assert polish.apply(allele, calls, sites, ins) == "aTgt" + "GG" + "A" + "A" + "GT" + "acg" + "C"
    assert polish.apply(allele, np.full(len(allele), polish.KEEP), sites, ins) == allele
    assert polish.apply("", [], sites, ins) == ""


def test_the_columns_and_their_round_trip():
    assert polish.COLUMNS == realign.COLUMNS + ("VaPoR_RA_PN", "VaPoR_RA_PCOV", "VaPoR_RA_PSUB", "VaPoR_RA_PDEL", "VaPoR_RA_PINS", "VaPoR_RA_PID")
    assert [i[0] for i in polish.INFO] == list(polish.COLUMNS) and all(len(i) == 4 for i in polish.INFO)
    assert polish.columns(None) == ["."] * 13 and polish.pack(None) == [] and polish.unpack([]) is None
    p = realign.Payload([12, -15, 3, 11])
    assert polish.columns(p) == realign.columns(p) + ["."] * 6                    # (no pile made)
    p.polish = polish.Polish([0, 2, 1200, 3, 5, 2, 4, 0], "ACGT")
    assert polish.columns(p) == realign.columns(p) + ["2", "1200", "3", "5", "4", "%.4f" % (1 - 12 / 1200)]
    q = polish.unpack(polish.pack(p))
    assert list(q) == list(p) and q.polish.stats == p.polish.stats and q.polish.text is None and polish.columns(q) == polish.columns(p)
    bare = polish.unpack(polish.pack(realign.Payload([1, 2])))
    assert list(bare) == [1, 2] and bare.polish is None
    p.polish = polish.Polish([0, 0, 0, 0, 0, 0, 0, 0])
    assert polish.columns(p)[-6:] == ["0", "0", "0", "0", "0", "."]              # PCOV == 0: no identity
    p.polish = polish.Polish([L.E_NOMEM, 0, 0, 0, 0, 0, 0, 0])
    assert polish.columns(p)[-6:] == ["."] * 6 and polish.columns(polish.unpack(polish.pack(p)))[-6:] == ["."] * 6
    assert polish.columns_many([None, p]) == [polish.columns(None), polish.columns(p)]
    assert polish.identity([0, 3, 7, 1, 0, 0, 0, 0]) == "0.8571"


def test_the_writer_adds_the_polished_alleles(tmp_path):
    def payload(text):
        p = realign.Payload([20])
        p.traces = realign.Traces("ACGTACGT", "ACGT", [("ACGT", 0, 4, 0, 4, 4, [(4, "=")])])
        p.polish = polish.Polish([0, 1, 0, 0, 0, 0, 0, 0], text)
        return p
    plain = realign.TraceWriter(str(tmp_path / "p"))
    w = polish.PolishWriter(str(tmp_path / "o"))
    for sink in (plain, w):
        sink.take(5, "k:2", payload("ACGA"))
        sink.take(1, "k:1", payload("ACT"))
        sink.take(3, "k:1", payload("ACGT"))
        sink.take(2, "none", None)
    plain.close()
    assert w.close() == (str(tmp_path / "o.sam"), str(tmp_path / "o.fa"), str(tmp_path / "o.pol.fa"))
    assert (tmp_path / "o.pol.fa").read_text() == ">k:1|POL\nACT\n>k:1#2|POL\nACGT\n>k:2|POL\nACGA\n"
    for ext in (".sam", ".fa"):
        assert (tmp_path / ("o" + ext)).read_text() == (tmp_path / ("p" + ext)).read_text()
    assert polish.PolishWriter(str(tmp_path / "o"), 2, 4).close()[2] == str(tmp_path / "o.rank2.pol.fa")


# ------------------------------------------------------------------------------------------------------------------------------
# the parser
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_flag_parses_and_the_help_text_is_unchanged(monkeypatch):
    p = cli.build_parser()
    assert p.parse_args(TR.BASE + ["--realign", "--realign-polish"]).realign_polish is True and p.parse_args(TR.BASE).realign_polish is False
    assert p.parse_args(TR.BASE + ["--realign", "--realign-polish", "--realign-out", "pre"]).realign_out == "pre"
    assert "--realign-polish" not in cli.MODE_OPTIONS and len(cli.MODE_OPTIONS) == 9
    monkeypatch.setenv("COLUMNS", "80")
    with open(os.path.join(ROOT, "tests", "golden", "cli_help.txt")) as f:
        assert p.format_help() == f.read()
    assert "--realign-polish" not in p.format_help() and "--realign-polish" not in p.format_usage()
    assert modes.REALIGN.COLUMNS == realign.COLUMNS


def test_refused_without_realign(capsys):
    for cmd in ("bed", "vcf", "svelter", "ins"):
        TR._refused([cmd] + TR.BASE + ["--realign-polish"], "--realign-polish needs --realign", capsys)
    TR._refused(["bed"] + TR.BASE + ["--realign-polish", "--support"], "--realign-polish needs --realign", capsys)


# ------------------------------------------------------------------------------------------------------------------------------
# the entry, its binding and the host plan of the call
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_is_declared_exported_and_bound():
    h = open(os.path.join(ROOT, "include", "vapor_hip.h")).read()
    assert re.search(r"\bint vapor_realign_polish\(vapor_ctx\* ctx, vapor_seqset\* set, int64_t n_pairs, const vapor_pair\* pairs, int32_t band, "
                     r"int64_t n_loci,\s+const int64_t\* first, const int64_t\* col_off, int32_t\* stats, uint8_t\* calls, int32_t\* sites, "
                     r"uint8_t\* ins,\s+uint32_t\* counts\);", h)
    assert "vapor_realign_polish" in L.EXPORTS and "vapor_realign_polish" in L.OPTIONAL_EXPORTS and L.ABI_VERSION == 3
    lib = L.load()
    assert hasattr(lib, "vapor_realign_polish") and len(lib.vapor_realign_polish.argtypes) == 13
    from vapor_amd import build
    assert any(p.endswith("vapor_polish.h") for p in build.KERNEL_FILES) and any(p.endswith("vapor_polish_plan.h") for p in build.DEPS)
    stub = open(os.path.join(ROOT, "vapor_amd", "csrc", "vapor_bam.cpp")).read()
    assert re.search(r'__attribute__\(\(weak\)\) int vapor_realign_polish\(', stub)


def test_an_engine_without_the_entry_raises_one_clear_error(monkeypatch):
    from vapor_amd.engine import Engine

    class Without:
        def vapor_build_flags(self):
            return b""
    monkeypatch.setattr(L, "load", lambda: Without())
    e = object.__new__(Engine)
    assert e.realign_polish_available() is False
    with pytest.raises(NotImplementedError, match=r"vapor_realign_polish: the loaded library has no pileup kernels \(--realign-polish\)"):
        Engine.realign_polish(e, None, np.zeros(0, dtype=L.PAIR_DTYPE), 256, [0], [0])


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("polish") / "polish_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "vapor_amd", "csrc"),
                           os.path.join(ROOT, "tools", "polish_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("line", [
    "constants and layout: stated",
    "tables: 2000 calls, refused ones among them",
    "locus status: 3000 loci, every status met",
    "groups: 400 calls, many in several groups",
    "call plan: 66 calls, every kind of locus, many in several groups; check_args: 172 cases",
    "polish_check: all equal",
])
def test_the_calls_host_plan_against_direct_statements_under_sanitizers(check_output, line):
    assert line in check_output


# ------------------------------------------------------------------------------------------------------------------------------
# through cli.main, on an engine whose distances, traces and piles are the statements'
# ------------------------------------------------------------------------------------------------------------------------------
_POLISHED = {}


def stated_polish(self, ss, pairs, band, first, col_off, want_counts=False):
    """Engine.realign_polish by polish.statement over the set's texts (`texts` where the stand-in keeps the derived ones there)."""
    texts = getattr(ss, "texts", None) or ss.seqs
    ng = len(first) - 1
    stats = np.zeros((ng, 8), dtype=np.int32)
    calls = np.zeros(int(col_off[-1]), dtype=np.uint8)
    sites = np.zeros((ng, polish.MAX_SITES, 2), dtype=np.int32)
    ins = np.zeros((ng, polish.MAX_SITES, polish.RMAX), dtype=np.uint8)
    for g in range(ng):
        mine = pairs[first[g]:first[g + 1]]
        n_col = col_off[g + 1] - col_off[g]
        if not len(mine):
            calls[col_off[g]:col_off[g + 1]] = polish.KEEP
            continue
        allele = texts[mine[0]["seq2"]]
        assert len(allele) == n_col and all(p["seq2"] == mine[0]["seq2"] for p in mine)
        key = (tuple((texts[p["seq1"]], int(p["off2"])) for p in mine), allele, band)
        if key not in _POLISHED:
            _POLISHED[key] = polish.statement(list(key[0]), allele, band)
        _counts, calls[col_off[g]:col_off[g + 1]], sites[g], ins[g], stats[g] = _POLISHED[key]
    return stats, calls, sites, ins, None


class PolishFake(TT.TraceFake):
    """TraceFake plus realign_polish: the statement over the set's texts; records what it was asked."""

    def __init__(self, orc):
        super().__init__(orc)
        self.polish_calls = []           # per call: (pairs, loci)

    def realign_polish(self, ss, pairs, band, first, col_off, want_counts=False):
        self.polish_calls.append((len(pairs), len(first) - 1))
        return stated_polish(self, ss, pairs, band, first, col_off, want_counts)


@pytest.fixture()
def fake(oracle):
    eng = PolishFake(oracle)
    pipeline.set_engine(eng)
    yield eng
    pipeline.set_engine(None)
    seqio.set_backend(None)


SPECS = TT.SPECS


def test_cli_on_a_world_in_memory(fake, tmp_path):
    w = synth.make_support_world(seed=4, specs=SPECS, layers=4, read_len=4000)
    text = synth.bed_text(w)
    seqio.set_backend(seqio.MemorySamtools(w))
    pre = str(tmp_path / "ra_pre")
    plain, _ = TS.run_main(tmp_path, "ra", "bed", text, ["--realign", "--realign-out", pre])
    assert fake.realign_calls and fake.trace_calls and not fake.polish_calls       # no realign_polish call without the flag
    files = {}
    for name, more in (("whole", []), ("one", ["--chunk", "1"])):
        fake.polish_calls.clear()
        seqio.set_backend(seqio.MemorySamtools(w))
        p = str(tmp_path / (name + "_pre"))
        table, _ = TS.run_main(tmp_path, name, "bed", text, ["--realign", "--realign-polish", "--realign-out", p] + more)
        assert fake.polish_calls
        files[name] = (table, open(p + ".sam").read(), open(p + ".fa").read(), open(p + ".pol.fa").read())
    assert files["whole"] == files["one"]                                          # neither threads nor chunking show
    table, sam, fa, pol = files["whole"]
    assert sam == open(pre + ".sam").read() and fa == open(pre + ".fa").read()     # --realign-out's files, byte for byte
    rows = [r.split("\t") for r in table.splitlines()]
    assert rows[0][-13:] == list(polish.COLUMNS)
    assert "\n".join("\t".join(r[:-6]) for r in rows) + "\n" == plain               # --realign's columns, followed by the six
    # PREFIX.pol.fa: one entry a locus with a payload, in job order, the statement's text
    names = [ln[1:-4] for ln in fa.splitlines()[0::4]]
    alts = fa.splitlines()[3::4]
    assert pol.splitlines()[0::2] == [">%s|POL" % n for n in names] and len(names) == len(SPECS)
    reads_of = {}
    for ln in sam.splitlines():
        f = ln.split("\t")
        if not ln.startswith("@") and f[14] == "vt:Z:ALT":
            reads_of.setdefault(f[0].rsplit("/", 1)[0], []).append(f)
    for r, name, alt, text_pol in zip(rows[1:], names, alts, pol.splitlines()[1::2]):
        n_alt = int(r[-13])
        assert r[-6] == str(n_alt)                                                 # the reads piled are the ALT voters
        if n_alt == 0:
            assert r[-6:] == ["0", "0", "0", "0", "0", "."] and text_pol == alt
    # exact calls polish to an identity of 1.0000 on the hom loci
    # (the INS world's allele is built one base beside the planted one: its pile says so with a single edit)
    hom = [r for r, (t, _s, z) in zip(rows[1:], SPECS) if z == "hom" and t != "INS"]
    assert len(hom) == 3 and all(r[-1] == "1.0000" and r[-4:-1] == ["0", "0", "0"] and int(r[-5]) > 0 for r in hom), [r[-6:] for r in hom]
    for r in rows[1:]:
        if r[-6] != ".":
            pn, pcov, psub, pdel, pins = (int(v) for v in r[-6:-1])
            assert r[-1] == (polish.identity([0, pn, pcov, psub, pdel, 0, pins, 0]) or "."), r[-6:]
    # a locus without a payload: '.' in all thirteen, and nothing written
    seqio.set_backend(seqio.MemorySamtools(w))
    p = str(tmp_path / "few_pre")
    few, _ = TS.run_main(tmp_path, "few", "bed", text, ["--realign", "--realign-polish", "--realign-out", p, "--PB-supp", "1000"])
    assert all(r.split("\t")[-13:] == ["."] * 13 for r in few.splitlines()[1:]) and open(p + ".pol.fa").read() == ""
    # without --realign-out: the same table, no files
    seqio.set_backend(seqio.MemorySamtools(w))
    bare, _ = TS.run_main(tmp_path, "bare", "bed", text, ["--realign", "--realign-polish"])
    assert bare == table


def test_a_world_whose_calls_are_shifted_polishes_to_the_shift(fake, tmp_path):
    """DEL calls whose end is 5 bases off: the alt allele built from them lacks 5 bases the reads carry (or carries 5 they lack);
    the polish reports them at the junction.  Asserted against the statement's own answer through the files: the polished
    allele realigns the ALT voters with fewer edits."""
    w = synth.make_support_world(seed=4, specs=SPECS[:1], layers=4, read_len=4000)
    lines = synth.bed_text(w).splitlines()
    shifted = []
    for ln in lines:
        f = ln.split("\t")
        f[2] = str(int(f[2]) + 5)
        shifted.append("\t".join(f))
    seqio.set_backend(seqio.MemorySamtools(w))
    p = str(tmp_path / "s_pre")
    table, _ = TS.run_main(tmp_path, "s", "bed", "\n".join(shifted) + "\n", ["--realign", "--realign-polish", "--realign-out", p])
    r = table.splitlines()[1].split("\t")
    pn, pcov, psub, pdel, pins = (int(v) for v in r[-6:-1])
    assert pn >= 3 and pcov > 0 and 3 <= pdel + pins + psub <= 10 and pdel + pins >= 3, r[-6:]
    assert r[-1] == polish.identity([0, pn, pcov, psub, pdel, 0, pins, 0]) != "1.0000"
    # the statement's answer for this very locus, from the files
    fa, sam = open(p + ".fa").read().splitlines(), open(p + ".sam").read().splitlines()
    alt = fa[3]
    voters = [ln.split("\t") for ln in sam if not ln.startswith("@") and ln.split("\t")[14] == "vt:Z:ALT"]
    assert len(voters) == pn
    pol = open(p + ".pol.fa").read().splitlines()[1]
    assert len(pol) == len(alt) - pdel + pins
    # the polished allele is the sequence the reads carry: every voter aligns to it with fewer edits, the 5 bases gone
    for f in voters[:4]:
        off = min(int(f[3]) - 1, len(pol))
        before = realign.statement(f[9], alt, min(int(f[3]) - 1, len(alt)), realign.BAND)
        after = realign.statement(f[9], pol, off, realign.BAND)
        assert after <= before - 3, (before, after)

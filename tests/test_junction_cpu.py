"""`--realign-junction` without a device: the numpy statement (junction.row_table, junction, lens) against the
plain-integer model (tests/junction_model.py) on every designed case and 60 fuzz pairs, the model's nine mutants every one of
which those cases tell from the rule at least three times, the columns and their round trip, the parser, the header's prototype
and the export lists, the host plan of the call under the sanitizers as a program of its own (tools/junction_check.cpp), and
cli.main on an engine whose four realign entries are the statements."""
import os
import re
import subprocess

import numpy as np
import pytest

import junction_model as M
import test_polish_cpu as TP
import test_realign_cpu as TR
import test_signature_cpu as TS
from conftest import ROOT
from vapor_amd import _lib as L
from vapor_amd import cli, junction, modes, pipeline, polish, realign, seqio, synth


# ------------------------------------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------------------------------------
def stated(s, l, band):
    """junction.junction in the model's shape."""
    got, rows = junction.junction(s.decode("latin-1"), l.decode("latin-1"), band, True)
    return got, [tuple(r) for r in rows.tolist()]


def test_the_statement_equals_the_model_on_every_designed_pair():
    pairs, expect = M.designed_pairs(), M.expected_pairs()
    assert len(pairs) >= 80 and {len(p[1]) for p in pairs} >= set(M.LENGTHS)
    wrong = [(name, stated(s, l, band)[0], e[0]) for (name, s, l, band), e in zip(pairs, expect) if stated(s, l, band) != e]
    assert not wrong, (len(wrong), wrong[:3])
    for name, s, l, band in pairs[::7]:                        # row_table is the forward pass's half of the rows
        f, jf = junction.row_table(s.decode("latin-1"), l.decode("latin-1"), band)
        assert list(zip(f.tolist(), jf.tolist())) == M.row_table(s, l, band), name


def test_the_statement_equals_the_model_on_the_fuzz():
    pairs = M.fuzz_pairs()
    assert len(pairs) == 60 and all(len(s) <= len(l) for _n, s, l, _b in pairs)
    for name, s, l, band in pairs:
        assert stated(s, l, band) == M.junction(s, l, band), name


def test_lens_and_the_gate_equal_the_model_on_every_designed_locus():
    for name, called, polished, window, band in M.designed_loci():
        c, p, w = (v.decode("latin-1") for v in (called, polished, window))
        for allele, raw in ((c, called), (p, polished)):
            cost, left, right, glen, kind = junction.lens(allele, w, band)
            assert (cost, left, right, glen, junction.TYPES[kind]) == M.lens(raw, window, band), name
        # the columns, through a payload as the pipeline makes it
        pay = realign.Payload([20, 20, 20])
        pay.polish = polish.Polish([0, 3, 100, 0, 0, 0, 0, 0])
        pay.junction = junction.Junction(junction.lens(c, w, band)[:4] + junction.lens(p, w, band))
        assert junction.six(pay) == (M.locus(called, polished, window, band) or ["."] * 6), name


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_mutant_is_told_from_the_rule_by_three_designed_cases(mutant):
    assert len(M.MUTANTS) == 9
    assert M.told_apart(mutant) >= 3, (mutant, M.told_apart(mutant))


def test_the_designed_cases_the_section_names_are_there():
    by = dict(zip((p[0] for p in M.designed_pairs()), M.expected_pairs()))
    # a planted jump comes back exactly, whether the two passes' bands overlap (jump <= 2B) or not, at any length
    for band in (1, 2, 31, 32, 33, 100):
        for jump in (1, band, band + 1, 2 * band, 2 * band + 1, 1000):
            cost, _i, j1, j2, _f, _r = by["jump of %d B=%d" % (jump, band)][0]
            assert (cost, j2 - j1) == (0, jump), (jump, band)
    for name in ("jump of 256 B=256", "jump of 513 B=256", "jump of 1024 B=512", "jump of 1025 B=512"):
        assert by[name][0][0] == 0 and by[name][0][3] - by[name][0][2] == int(name.split()[2])
    # microhomology: left-normalised, the same row whatever the homology's length
    assert [by["microhomology of %d" % h][0][:3] for h in (0, 1, 5)] == [(0, 20, 20)] * 3
    assert [by["microhomology of %d" % h][0][3] for h in (0, 1, 5)] == [33, 34, 38]
    assert by["jump at row 0"][0][:4] == (0, 0, 0, 12) and by["jump at row ns"][0][:4] == (0, 60, 60, 72)
    for name in ("substitution left of the jump", "substitution right of the jump", "insertion beside the jump", "deletion beside the jump"):
        assert by[name][0][0] == 1, name
    # N matches nothing, not even itself; an inverted segment has no one-jump reading
    assert by["N in both, no jump"][0][0] == 2 and by["N on both sides of the jump"][0][0] == 1
    assert by["inverted segment"][0][0] > 10
    assert sum(1 for p in M.designed_pairs() if p[0].startswith("validity pair")) >= 6
    assert all(len(s) <= 14 and len(l) <= 14 and set(s + l) <= set(b"AC") for n, s, l, _b in M.designed_pairs() if n.startswith("validity pair"))
    loci = {l[0]: M.locus(*l[1:]) for l in M.designed_loci()}
    for name, glen in (("exact DEL", 50), ("exact INS", 40), ("exact TANDUP", 50)):
        assert loci[name] == [name.split()[1].replace("TANDUP", "INS"), str(glen), str(glen), "0", "0", "0"]
    assert int(loci["DEL called 5 late"][2]) - int(loci["DEL called 5 late"][1]) == 5
    assert all(loci["INV %d" % k] is None for k in range(3)) and loci["window with N outside the jump"] is None


def test_the_columns_and_their_round_trip():
    assert junction.COLUMNS == polish.COLUMNS + ("VaPoR_RA_JT", "VaPoR_RA_JLEN", "VaPoR_RA_JLEN0", "VaPoR_RA_JDL", "VaPoR_RA_JDR", "VaPoR_RA_JCOST")
    assert [i[0] for i in junction.INFO] == list(junction.COLUMNS) and all(len(i) == 4 for i in junction.INFO)
    assert junction.INFO[:len(polish.INFO)] == polish.INFO
    assert junction.columns(None) == ["."] * 19 and junction.pack(None) == [] and junction.unpack([]) is None
    p = realign.Payload([12, -15, 30, 11])
    assert junction.columns(p) == polish.columns(p) + ["."] * 6                  # (no pile, no junction)
    p.polish = polish.Polish([0, 3, 1200, 3, 5, 2, 4, 0], "ACGT")
    assert junction.columns(p) == polish.columns(p) + ["."] * 6                  # (a pile, no junction: a pair came back with a status)
    p.junction = junction.Junction([0, 100, 155, 55, 2, 101, 151, 50, junction.DEL])
    assert junction.columns(p) == polish.columns(p) + ["DEL", "50", "55", "1", "-4", "2"]
    q = junction.unpack(junction.pack(p))
    assert list(q) == list(p) and q.polish.stats == p.polish.stats and q.junction.vals == p.junction.vals
    assert junction.columns(q) == junction.columns(p)
    # the gates: a status, fewer than MIN_COV reads piled, a call's allele that is no single jump
    for stats, vals in (([L.E_NOMEM, 3, 0, 0, 0, 0, 0, 0], p.junction.vals), ([0, 2, 1200, 0, 0, 0, 0, 0], p.junction.vals),
                        ([0, 3, 1200, 0, 0, 0, 0, 0], (1,) + p.junction.vals[1:])):
        g = realign.Payload([12, 30, 11])
        g.polish, g.junction = polish.Polish(stats), junction.Junction(vals)
        assert junction.six(g) == ["."] * 6 and junction.six(junction.unpack(junction.pack(g))) == ["."] * 6, stats
    # without a pile, and with a pile but no junction, the flags keep their places
    bare = junction.unpack(junction.pack(realign.Payload([1, 2])))
    assert list(bare) == [1, 2] and bare.polish is None and bare.junction is None
    p.junction = None
    half = junction.unpack(junction.pack(p))
    assert half.polish.stats == p.polish.stats and half.junction is None
    assert junction.columns_many([None, p]) == [junction.columns(None), junction.columns(p)]
    p.junction = junction.Junction([0, 90, 90, 40, 0, 90, 90, 0, junction.NONE])
    assert junction.six(p) == ["NONE", "0", "40", "0", "0", "0"]
    with pytest.raises(ValueError):
        junction.Junction([0] * 8)


# ------------------------------------------------------------------------------------------------------------------------------
# the parser
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_flag_parses_and_the_help_text_is_unchanged(monkeypatch):
    p = cli.build_parser()
    full = TR.BASE + ["--realign", "--realign-polish", "--realign-junction"]
    assert p.parse_args(full).realign_junction is True and p.parse_args(TR.BASE + ["--realign", "--realign-polish"]).realign_junction is False
    assert p.parse_args(full + ["--realign-out", "pre"]).realign_out == "pre"
    assert "--realign-junction" not in cli.MODE_OPTIONS and len(cli.MODE_OPTIONS) == 9
    monkeypatch.setenv("COLUMNS", "80")
    with open(os.path.join(ROOT, "tests", "golden", "cli_help.txt")) as f:
        assert p.format_help() == f.read()
    assert "--realign-junction" not in p.format_help() and "--realign-junction" not in p.format_usage()
    assert modes.REALIGN.COLUMNS == realign.COLUMNS


def test_refused_without_realign_polish(capsys):
    for cmd in ("bed", "vcf", "svelter", "ins"):
        TR._refused([cmd] + TR.BASE + ["--realign-junction"], "--realign-junction needs --realign-polish", capsys)
    TR._refused(["bed"] + TR.BASE + ["--realign", "--realign-junction"], "--realign-junction needs --realign-polish", capsys)
    TR._refused(["vcf"] + TR.BASE + ["--realign", "--realign-out", "pre", "--realign-junction"], "--realign-junction needs --realign-polish", capsys)


# ------------------------------------------------------------------------------------------------------------------------------
# the entry, its binding and the host plan of the call
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_is_declared_exported_and_bound():
    h = open(os.path.join(ROOT, "include", "vapor_hip.h")).read()
    assert re.search(r"\bint vapor_realign_junction\(vapor_ctx\* ctx, vapor_seqset\* set, int64_t n_pairs, const vapor_pair\* pairs, int32_t band, "
                     r"int32_t\* out,\s+const int64_t\* row_off, int32_t\* rows\);", h)
    assert "vapor_realign_junction" in L.EXPORTS and "vapor_realign_junction" in L.OPTIONAL_EXPORTS and L.ABI_VERSION == 3
    lib = L.load()
    assert hasattr(lib, "vapor_realign_junction") and len(lib.vapor_realign_junction.argtypes) == 8
    from vapor_amd import build
    assert any(p.endswith("vapor_junction.h") for p in build.KERNEL_FILES) and any(p.endswith("vapor_junction_plan.h") for p in build.DEPS)
    stub = open(os.path.join(ROOT, "vapor_amd", "csrc", "vapor_bam.cpp")).read()
    assert re.search(r'__attribute__\(\(weak\)\) int vapor_realign_junction\(', stub)


def test_an_engine_without_the_entry_raises_one_clear_error(monkeypatch):
    from vapor_amd.engine import Engine

    class Without:
        def vapor_build_flags(self):
            return b""
    monkeypatch.setattr(L, "load", lambda: Without())
    e = object.__new__(Engine)
    assert e.realign_junction_available() is False
    with pytest.raises(NotImplementedError, match=r"vapor_realign_junction: the loaded library has no junction kernels \(--realign-junction\)"):
        Engine.realign_junction(e, None, np.zeros(0, dtype=L.PAIR_DTYPE), 256)


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("junction") / "junction_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "vapor_amd", "csrc"),
                           os.path.join(ROOT, "tools", "junction_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("line", [
    "layout and keys: stated, 4590 keys",
    "pairs: 24000 cases, every refusal met",
    "workspace: 2000 calls, some over the budget",
    "row tables: 2000 calls, refused ones and short slots among them",
    "junction_check: all equal",
])
def test_the_calls_host_plan_against_direct_statements_under_sanitizers(check_output, line):
    assert line in check_output


# ------------------------------------------------------------------------------------------------------------------------------
# through cli.main, on an engine whose distances, traces, piles and junctions are the statements'
# ------------------------------------------------------------------------------------------------------------------------------
_JUNCTIONS = {}


def stated_junction(self, ss, pairs, band, want_rows=False):
    """Engine.realign_junction by junction.junction over the set's texts (`texts` where the stand-in keeps the derived ones there)."""
    texts = getattr(ss, "texts", None) or ss.seqs
    out = np.zeros((len(pairs), 8), dtype=np.int32)
    for t, p in enumerate(pairs):
        s, l = texts[p["seq1"]], texts[p["seq2"]]
        if int(p["off2"]) != 0 or len(s) > len(l):
            out[t, 0] = L.E_ARG
            continue
        key = (s, l, band)
        if key not in _JUNCTIONS:
            _JUNCTIONS[key] = junction.junction(s, l, band)
        out[t, 1:7] = _JUNCTIONS[key]
    return out, None, None


class JunctionFake(TP.PolishFake):
    """PolishFake plus realign_junction: the statement over the set's texts; records what it was asked."""

    def __init__(self, orc):
        super().__init__(orc)
        self.junction_calls = []         # per call: (pairs, derived sequences of its set)

    def realign_junction(self, ss, pairs, band, want_rows=False):
        self.junction_calls.append((len(pairs), ss.n_derived))
        return stated_junction(self, ss, pairs, band, want_rows)


@pytest.fixture()
def fake(oracle):
    eng = JunctionFake(oracle)
    pipeline.set_engine(eng)
    yield eng
    pipeline.set_engine(None)
    seqio.set_backend(None)


SPECS = TP.SPECS
ALL = ["--realign", "--realign-polish", "--realign-junction"]


def test_cli_on_a_world_in_memory(fake, tmp_path):
    w = synth.make_support_world(seed=4, specs=SPECS, layers=4, read_len=4000)
    text = synth.bed_text(w)
    seqio.set_backend(seqio.MemorySamtools(w))
    pre = str(tmp_path / "po_pre")
    polished, _ = TS.run_main(tmp_path, "po", "bed", text, ["--realign", "--realign-polish", "--realign-out", pre])
    assert fake.polish_calls and not fake.junction_calls                           # no realign_junction call without the flag
    tables = {}
    for name, more in (("whole", []), ("one", ["--chunk", "1"]), ("files", ["--realign-out", str(tmp_path / "ju_pre")])):
        fake.junction_calls.clear()
        seqio.set_backend(seqio.MemorySamtools(w))
        tables[name], _ = TS.run_main(tmp_path, name, "bed", text, ALL + more)
        assert fake.junction_calls and all(n % 2 == 0 for n, _d in fake.junction_calls)     # two pairs a locus
    assert tables["whole"] == tables["one"] == tables["files"]                     # neither threads, chunking nor a sink show
    for ext in (".sam", ".fa", ".pol.fa"):                                         # --realign-out's three files, byte for byte
        assert open(str(tmp_path / "ju_pre") + ext).read() == open(pre + ext).read(), ext
    rows = [r.split("\t") for r in tables["whole"].splitlines()]
    assert rows[0][-19:] == list(junction.COLUMNS)
    assert "\n".join("\t".join(r[:-6]) for r in rows) + "\n" == polished            # --realign-polish's columns, followed by the six
    assert len(rows) == 1 + len(SPECS)
    for r, (kind, size, zyg) in zip(rows[1:], SPECS):
        six, pn = r[-6:], r[-12]
        if kind == "INV" or pn == "." or int(pn) < polish.MIN_COV:
            assert six == ["."] * 6, (kind, zyg, r[-12:])                          # no single jump, or fewer than three piled reads
        elif zyg == "hom" and kind != "INS":
            # exact DEL and TANDUP calls: the polished allele's jump is the call's own
            # (an exact INS call has a test of its own below)
            assert six == ["DEL" if kind == "DEL" else "INS", str(size), str(size), "0", "0", "0"], (kind, r[-12:])
        elif zyg == "hom":
            # the INS world's call carries the planted text whole, and vapor_simple_ins repeats the base at the insertion point:
            # the call's allele is one base longer than what the reads carry (test_polish_cpu: PDEL = 1), and the lens says so
            assert six[0] == "INS" and (int(six[1]), int(six[2])) == (size, size + 1) and six[3] == six[4] and six[5] == "0", r[-12:]
    assert any(r[-6:] == ["."] * 6 and r[-12] not in (".",) for r in rows[1:])      # a locus with a pile and no lens is among them
    assert sum(1 for r in rows[1:] if r[-6] != ".") >= 3
    # a locus without a payload: '.' in all nineteen
    seqio.set_backend(seqio.MemorySamtools(w))
    fake.junction_calls.clear()
    few, _ = TS.run_main(tmp_path, "few", "bed", text, ALL + ["--PB-supp", "1000"])
    assert all(r.split("\t")[-19:] == ["."] * 19 for r in few.splitlines()[1:]) and not fake.junction_calls


def test_an_exact_ins_call_reads_as_itself_through_the_cli(fake, tmp_path):
    """An exact INS call at JDL = JDR = 0, JLEN == JLEN0, JCOST = 0 through cli.main.  vapor_simple_ins builds the alt allele as
    flank + ins + flank with the base at the insertion point in both flanks (SF:1872), so a call is exact - the allele is what
    the reads carry, the polish finds nothing - when its text followed by that base is the inserted sequence: in the world of
    seed 1 the planted insertion ends with that base, and the call is the planted text without it.  The lens reads the allele
    on the stretch of the window it spans (pipeline._lens_window): the window itself runs len(ins) bases further."""
    w = synth.make_support_world(seed=1, specs=(("INS", 250, "hom"),), layers=4, read_len=4000)
    f = synth.bed_text(w).splitlines()[0].split("\t")
    f[5] = f[5][:-1]
    seqio.set_backend(seqio.MemorySamtools(w))
    table, _ = TS.run_main(tmp_path, "ins", "bed", "\t".join(f) + "\n", ALL)
    r = table.splitlines()[1].split("\t")
    print("INS through the CLI:", r[-12:])
    assert r[-10:-7] == ["0", "0", "0"] and r[-7] == "1.0000", r[-12:]             # (the call is exact: nothing to polish)
    kind, jlen, jlen0, jdl, jdr, jcost = r[-6:]
    assert kind == "INS" and jlen == jlen0 == "250" and (jdl, jdr, jcost) == ("0", "0", "0"), r[-12:]


def test_an_exact_insertion_reads_as_itself(fake, tmp_path):
    """An INS call whose allele is the planted one: JDL = JDR = 0, JLEN == JLEN0, JCOST = 0 - stated on the lens directly, with
    the polished allele the call's own, as an exact call polishes (test_polish_cpu: identity 1.0000)."""
    rng = np.random.default_rng(8)
    w = "".join("ACGT"[j] for j in rng.integers(0, 4, 900))
    ins = "".join("ACGT"[j] for j in rng.integers(0, 4, 250))
    alt = w[:400] + ins + w[400:]
    pay = realign.Payload([200, 210, 190])
    pay.polish = polish.Polish([0, 3, len(alt), 0, 0, 0, 0, 0])
    pay.junction = junction.Junction(junction.lens(alt, w, realign.BAND)[:4] + junction.lens(alt, w, realign.BAND))
    assert junction.six(pay) == ["INS", "250", "250", "0", "0", "0"]


def test_a_call_that_ends_5_bases_late_reads_5_bases_longer(fake, tmp_path):
    """test_polish_cpu's world whose DEL call ends 5 bases late: the call's own jump is 5 bases longer than the jump of the
    allele the reads carry."""
    w = synth.make_support_world(seed=4, specs=SPECS[:1], layers=4, read_len=4000)
    shifted = []
    for ln in synth.bed_text(w).splitlines():
        f = ln.split("\t")
        f[2] = str(int(f[2]) + 5)
        shifted.append("\t".join(f))
    seqio.set_backend(seqio.MemorySamtools(w))
    table, _ = TS.run_main(tmp_path, "s", "bed", "\n".join(shifted) + "\n", ALL)
    r = table.splitlines()[1].split("\t")
    kind, jlen, jlen0, jdl, jdr, jcost = r[-6:]
    assert kind == "DEL" and int(jlen0) - int(jlen) == 5, r[-12:]
    assert int(jlen0) == SPECS[0][1] + 5 and int(jlen) == SPECS[0][1]
    assert int(jdr) - int(jdl) == -5 and int(jcost) == 0, r[-6:]

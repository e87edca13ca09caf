"""`--realign` without a device: the Python statement (realign.statement) against the plain-integer model
(tests/realign_model.py) on the designed cases, the mutants of the model every one of which those cases tell from the rule, the
mode's surface as cli.py and the VCF writer see it, the parser, the host arithmetic of the call under the sanitizers as a program
of its own (tools/realign_check.cpp), and the wrapper driver through cli.main on an engine whose distances are the statement's."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import realign_model as M
import test_signature_cpu as TS
from conftest import ROOT
from fake_engine import FakeEngine
from vapor_amd import _lib as L
from vapor_amd import cli, drivers, modes, pipeline, realign, seqio, support, synth
from vapor_amd import simple_function as SF


# ------------------------------------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_statement_equals_the_model_on_every_designed_case():
    cases, expect = M.designed_cases(), M.designed_expected()
    assert len(cases) == len(expect) > 450
    for (name, read, allele, off2, band), e in zip(cases, expect):
        assert realign.statement(read, allele, off2, band) == e, name
    for name, read, allele, off2, band in M.fuzz_cases():
        assert realign.statement(read.decode(), allele.decode(), off2, band) == M.distance(read, allele, off2, band), name


def test_designed_cases_by_hand():
    by = dict(zip((c[0] for c in M.designed_cases()), M.designed_expected()))
    assert by["identical B=1"] == 0 and by["first symbol B=32"] == 1 and by["last symbol B=100"] == 1
    for band in M.BANDS:
        # bridged at cost B, exactly; one more is not: the band has no path that takes the whole event
        assert by["insertion of %d B=%d" % (band, band)] == band and by["deletion of %d B=%d" % (band, band)] == band
        assert by["insertion of %d B=%d" % (band + 1, band)] > band + 1 and by["deletion of %d B=%d" % (band + 1, band)] > band + 1
    assert by["len n=0 m=0 B=1"] == 0 and by["len n=0 m=300 B=512"] == 0 and by["len n=300 m=0 B=512"] == 0
    assert by["N against N"] == 4 and by["IUPAC"] == 10 and by["lower IUPAC and n"] == 3 and by["lower against upper"] == 0
    assert by["a byte outside the alphabet"] == 2 and by["X against X"] == 8
    assert by["off2=8 == len(seq2)"] == 0 and by["n - m > B, B=31"] == 1 and by["m - n > B, B=31"] == 1


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_the_designed_cases_tell_every_mutant_from_the_rule(mutant):
    if mutant == "vote_strict":
        assert [M.vote(d) for d in M.VOTE_CASES] == ["ALT", "REF", None, None, "ALT", "REF", None]
        assert [M.vote(d, mutant) for d in M.VOTE_CASES] != [M.vote(d) for d in M.VOTE_CASES]
        return
    # (the designed cases of at most 20 000 cells are enough for every mutant, and quick)
    small = [(c, e) for c, e in zip(M.designed_cases(), M.designed_expected()) if len(c[1]) * len(c[2]) <= 20000]
    killed = [c[0] for c, e in small if M.distance(c[1], c[2], c[3], c[4], mutant) != e]
    assert killed, mutant


def test_votes_counts_and_genotype_are_the_models():
    assert realign.MARGIN == M.MARGIN == 10 and realign.BAND == 256 and realign.MAX_BAND == L.MAX_BAND == 512 and support.ERR == M.ERR
    diffs = realign.votes([30, 5, 14, 0, 50], [20, 15, 5, 0, 61])
    assert diffs == [10, -10, 9, 0, -11] and realign.counts(diffs) == (1, 2, 2)
    for diffs in ([], list(M.VOTE_CASES), [40] * 6, [-40] * 5, [40, 40, -40, -40, 3], [9, -9]):
        assert realign.columns(realign.Payload(diffs)) == M.columns(diffs), diffs
    for alt, ref in itertools.product(range(0, 9), repeat=2):
        assert support.genotype(alt, ref) == M.genotype(alt, ref)
    assert M.columns([40] * 6) == ["6", "0", "0", "1.000", "1/1", "16", "40,40,40,40,40,40"]
    assert M.columns([]) == ["0", "0", "0", ".", ".", ".", "."]
    assert realign.payload([5, 6], [1, 2], [0, 0], [0, L.E_ARG]) is None and realign.payload([5, 6], [1, 20]) == [4, -14]
    with pytest.raises(ValueError):
        realign.statement("ACGT", "ACGT", 0, 0)
    with pytest.raises(ValueError):
        realign.statement("ACGT", "ACGT", 5, 4)


# ------------------------------------------------------------------------------------------------------------------------------
# the mode's surface (as tests/test_modes_cpu.py holds the other seven)
# ------------------------------------------------------------------------------------------------------------------------------
def test_mode_surface():
    m = modes.REALIGN
    assert m.name == "realign" and m.attr == "realign" and m.skip_dot and not m.phased and m.chunk_gens is None and m.chunk_payloads is None
    assert m.pack(None) == [] and m.unpack(m.pack(None)) is None and m.unpack([]) is None
    for x in (realign.Payload([12, -30, 0, 9]), realign.Payload([]), realign.Payload([-131070])):
        flat = m.pack(x)
        assert flat and all(isinstance(v, float) for v in flat)
        back = m.unpack(flat)
        assert type(back) is realign.Payload and back == x
        assert len(m.columns_many([x, None])[0]) == len(m.COLUMNS)
    assert len(m.COLUMNS) == len(m.INFO) == len(m.keys) == len(m.columns_many([None])[0]) == 7
    assert m.columns_many([None])[0] == ["."] * 7
    assert [i[0] for i in m.INFO] == list(m.COLUMNS) == ["VaPoR_RA_ALT", "VaPoR_RA_REF", "VaPoR_RA_NC", "VaPoR_RA_VAF", "VaPoR_RA_GT",
                                                         "VaPoR_RA_GQ", "VaPoR_RA_Rec"]
    assert all(len(i) == 4 for i in m.INFO) and tuple(m.keys) == tuple(m.COLUMNS)


def test_info_lines_and_record_keys_of_the_annotated_vcf(tmp_path):
    m = modes.REALIGN
    vcf = tmp_path / "in.vcf"
    vcf.write_text('##fileformat=VCFv4.1\n##INFO=<ID=SVTYPE,Number=1,Type=String,Description="t">\n##source=x\n'
                   "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
                   "c1\t100\ta\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=500\nc1\t900\tb\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=990\n")
    values = ["v%d" % k for k in range(7)]
    table = "\t".join(["#CHR"] * 10 + list(m.COLUMNS)) + "\n"
    table += "\t".join(["c1:100:500:DEL", "0.5", "0.25", "0/1", "1.5", "0.5,-1.0"] + values) + "\n"
    table += "\t".join(["c1:900:990:DEL", "0.5", "0.25", "0/1", "1.5", "0.5,-1.0"] + ["."] * 7) + "\n"
    (tmp_path / "in.vcf.vapor").write_text(table)
    SF.vcf_vapor_modify(str(vcf), {"c1:100:500:DEL": [4], "c1:900:990:DEL": [5]}, mode=m)
    with_mode = (tmp_path / "in.vcf.vapor").read_text().splitlines()
    (tmp_path / "in.vcf.vapor").write_text(table)
    SF.vcf_vapor_modify(str(vcf), {"c1:100:500:DEL": [4], "c1:900:990:DEL": [5]})
    plain = (tmp_path / "in.vcf.vapor").read_text().splitlines()
    new = [ln for ln in with_mode if ln not in plain and ln.startswith("##")]
    at = with_mode.index(new[0])
    assert with_mode[at - 1].startswith("##INFO=<ID=VaPoR_REC,") and with_mode[at:at + len(new)] == new     # behind the row's own four
    got = [re.fullmatch(r'##INFO=<ID=(\w+),Number=([1.]),Type=(\w+),Description="([^"]+)">', ln).groups() for ln in new]
    assert [g[0] for g in got] == list(m.COLUMNS)
    assert {g[0] for g in got if g[1] == "."} == {"VaPoR_RA_Rec"}
    assert [g[2] for g in got] == ["Integer", "Integer", "Integer", "Float", "String", "Integer", "Integer"]
    assert all(g[3].endswith("(--realign)") for g in got)
    recs = [ln.split("\t") for ln in with_mode if not ln.startswith("#")]
    recs_plain = [ln.split("\t") for ln in plain if not ln.startswith("#")]
    assert len(recs) == 2 and [r[7] for r in recs_plain] == [r[7].split(";VaPoR_RA_ALT=")[0] for r in recs]
    assert recs[0][7][len(recs_plain[0][7]):] == "".join(";%s=%s" % kv for kv in zip(m.keys, values))
    assert recs[1][7][len(recs_plain[1][7]):] == ""


# ------------------------------------------------------------------------------------------------------------------------------
# the parser
# ------------------------------------------------------------------------------------------------------------------------------
BASE = ["--sv-input", "a.bed", "--reference", "r.fa", "--pacbio-input", "x.bam", "--output-path", "o", "--output-file", "o.vapor"]
OTHERS = {"--refine": ["--refine", "20"], "--phase-vcf": ["--phase-vcf", "p.vcf"], "--phased": ["--phased"], "--both-ends": ["--both-ends"],
          "--depth": ["--depth"], "--signatures": ["--signatures"], "--links": ["--links"], "--support": ["--support"]}


def _refused(argv, message, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and err.startswith("usage: vapor ") and err.endswith("\nvapor: error: %s\n" % message), (argv, err)


def test_the_option_parses_and_the_help_text_is_unchanged(monkeypatch):
    p = cli.build_parser()
    assert p.parse_args(BASE + ["--realign"]).realign is True and p.parse_args(BASE).realign is False
    assert cli.MODE_OPTIONS[-1] == "--realign" and len(cli.MODE_OPTIONS) == 9
    monkeypatch.setenv("COLUMNS", "80")
    with open(os.path.join(ROOT, "tests", "golden", "cli_help.txt")) as f:
        assert p.format_help() == f.read()
    assert "--realign" not in p.format_help() and "--realign" not in p.format_usage()


def test_refused_with_every_other_mode_option_in_both_orders(capsys):
    assert set(OTHERS) == set(cli.MODE_OPTIONS[:-1]) and len(OTHERS) == 8
    for other, given in OTHERS.items():
        spoken = "--realign and %s cannot be combined (a run has one mode)" % other
        for cmd in ("bed", "vcf"):
            _refused([cmd] + BASE + ["--realign"] + given, spoken, capsys)
            _refused([cmd] + BASE + given + ["--realign"], spoken, capsys)


def test_refused_outside_bed_and_vcf(capsys):
    for cmd in ("svelter", "ins"):
        _refused([cmd] + BASE + ["--realign"], "--realign applies to `vapor bed` and `vapor vcf`", capsys)


# ------------------------------------------------------------------------------------------------------------------------------
# the entry, its binding and the host arithmetic of the call
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_is_declared_exported_and_bound():
    h = open(os.path.join(ROOT, "include", "vapor_hip.h")).read()
    assert re.search(r"\bint vapor_realign_batch\(vapor_ctx\* ctx, vapor_seqset\* set, int64_t n_pairs, const vapor_pair\* pairs, int32_t band, int32_t\* out\);", h)
    assert "#define VAPOR_MAX_BAND 512" in h
    assert "vapor_realign_batch" in L.EXPORTS and "vapor_realign_batch" in L.OPTIONAL_EXPORTS and L.ABI_VERSION == 3
    lib = L.load()
    assert hasattr(lib, "vapor_realign_batch") and len(lib.vapor_realign_batch.argtypes) == 6


def test_an_engine_without_the_entry_raises_one_clear_error(monkeypatch):
    from vapor_amd.engine import Engine

    class Without:
        def vapor_build_flags(self):
            return b""
    monkeypatch.setattr(L, "load", lambda: Without())
    with pytest.raises(NotImplementedError, match=r"vapor_realign_batch: the loaded library has no realignment kernel \(--realign\)"):
        Engine.realign(object.__new__(Engine), None, np.zeros(0, dtype=L.PAIR_DTYPE), 256)


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("realign") / "realign_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "vapor_amd", "csrc"),
                           os.path.join(ROOT, "tools", "realign_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("line", [
    "bands: 519 values",
    "owners: 263168 slots of 512 bands, one owner each",
    "rows: 20000 cases",
    "pairs: 24000 cases, many refused",
    "launch: 7 sizes",
    "realign_check: all equal",
])
def test_the_calls_host_arithmetic_against_direct_statements_under_sanitizers(check_output, line):
    assert line in check_output


# ------------------------------------------------------------------------------------------------------------------------------
# the wrapper driver, through cli.main, on an engine whose distances are the statement's
# ------------------------------------------------------------------------------------------------------------------------------
_STATED = {}


class RealignFake(FakeEngine):
    """FakeEngine plus realign: the statement over the set's texts; records what it was asked."""

    def __init__(self, orc):
        super().__init__(orc)
        self.realign_calls = []          # per call: (pairs, derived sequences of its set, band)

    def realign(self, ss, pairs, band):
        self.realign_calls.append((len(pairs), ss.n_derived, band))
        d = np.zeros(len(pairs), dtype=np.int32)
        for t, p in enumerate(pairs):
            key = (ss.seqs[p["seq1"]], ss.seqs[p["seq2"]], int(p["off2"]), band)
            if key not in _STATED:                   # (the bed and the vcf run ask the same pairs)
                _STATED[key] = realign.statement(*key)
            d[t] = _STATED[key]
        return d, np.zeros(len(pairs), dtype=np.int32)


SPECS = (("DEL", 600, "hom"), ("DEL", 600, "ref"), ("DEL", 600, "het"), ("INS", 250, "hom"), ("INS", 250, "ref"), ("INV", 700, "hom"),
         ("TANDUP", 300, "hom"), ("DEL", 12000, "hom"))
WANT_GT = {"hom": "1/1", "ref": "0/0"}


@pytest.fixture()
def fake(oracle):
    eng = RealignFake(oracle)
    pipeline.set_engine(eng)
    yield eng
    pipeline.set_engine(None)
    seqio.set_backend(None)


def test_cli_on_a_world_in_memory(fake, tmp_path, monkeypatch):
    w = synth.make_support_world(seed=4, specs=SPECS, layers=4, read_len=4000)     # (reads long enough for the short windows)
    text = synth.bed_text(w)
    requests = []
    orig = pipeline.realign_requests
    monkeypatch.setattr(pipeline, "realign_requests", lambda eng, reqs: requests.append(len(reqs)) or orig(eng, reqs))
    seqio.set_backend(seqio.MemorySamtools(w))
    plain, _ = TS.run_main(tmp_path, "plain", "bed", text)
    assert not requests and not fake.realign_calls and "VaPoR_RA" not in plain
    seqio.set_backend(seqio.MemorySamtools(w))
    table, _ = TS.run_main(tmp_path, "ra", "bed", text, ["--realign"])
    rows = [r.split("\t") for r in table.splitlines()]
    assert rows[0][-7:] == list(realign.COLUMNS) and len(rows) == len(SPECS) + 1
    # the row's own columns are the plain run's, byte for byte
    assert "\n".join("\t".join(r[:-7]) for r in rows) + "\n" == plain
    # one Realign request a locus, one engine call a batch of them, alleles described (not uploaded), the command line's band
    assert sum(requests) == len(SPECS) and len(fake.realign_calls) == len(requests)
    assert all(nd >= 1 and band == realign.BAND and n % 2 == 0 for n, nd, band in fake.realign_calls)
    for r, (t, span, zyg) in zip(rows[1:], SPECS):
        alt, ref, nc, vaf, gt, gq, rec = r[-7:]
        diffs = [int(v) for v in rec.split(",")]
        assert r[-7:] == M.columns(diffs), (t, span, zyg)
        assert int(alt) + int(ref) + int(nc) == len(diffs) > 3
        if zyg in WANT_GT:
            assert gt == WANT_GT[zyg], (t, span, zyg, r[-7:])
    # a locus with too few reads makes no Score request: no Realign request, every column '.'
    requests.clear()
    seqio.set_backend(seqio.MemorySamtools(w))
    few, _ = TS.run_main(tmp_path, "few", "bed", text, ["--realign", "--PB-supp", "1000"])
    assert not requests and all(r.split("\t")[-7:] == ["."] * 7 for r in few.splitlines()[1:])
    # vcf: the same columns as INFO keys, the '.' ones left out; TANDUP is not scored by `vapor vcf`
    vtext = synth.vcf_text(w)
    seqio.set_backend(seqio.MemorySamtools(w))
    vplain, _ = TS.run_main(tmp_path, "vplain", "vcf", vtext)
    seqio.set_backend(seqio.MemorySamtools(w))
    vtable, annotated = TS.run_main(tmp_path, "vra", "vcf", vtext, ["--realign"])
    vrows = [r.split("\t") for r in vtable.splitlines()]
    assert "\n".join("\t".join(r[:-7]) for r in vrows) + "\n" == vplain
    by_chrom = {r[0].split(":")[0]: r[-7:] for r in vrows[1:]}
    bed_by_chrom = {r[0]: r[-7:] for r in rows[1:]}
    seen = [l for l in w.loci if l.svtype != "TANDUP"]
    assert len(by_chrom) == len(seen) == len(SPECS) - 1
    for l in seen:
        assert by_chrom[l.chrom] == bed_by_chrom[l.chrom], l
    lines = annotated.splitlines()
    assert sum(ln.startswith("##INFO=<ID=VaPoR_RA_") for ln in lines) == 7
    rec = {ln.split("\t")[2]: ln.split("\t")[7] for ln in lines if not ln.startswith("#")}
    assert set(rec) == {l.svid for l in seen}
    for l in seen:
        assert rec[l.svid].endswith("".join(";%s=%s" % kv for kv in zip(realign.COLUMNS, by_chrom[l.chrom]) if kv[1] != "."))


def test_the_wrapper_forwards_everything_and_asks_once():
    """vapor_realign around a driver that is a plain generator: every request goes through, every answer comes back - an
    exception as an exception - and the last Score request answered with a list is asked once more."""
    seen = []

    def driver(a, b):
        assert (a, b) == (1, 2)
        k = yield drivers.Window("W")
        seen.append(k)
        first = yield drivers.Score("s1", "REF1", "ALT1", [["r", 0, "q"]], 10)
        seen.append(first)
        try:
            yield drivers.Score("s2", "REF2", "ALT2", [["r", 1, "q"]], 10)
        except KeyError as e:
            seen.append(e)
        yield drivers.Figure([], "", 10, "R", "A", "name")
        return [0.5]

    gen = drivers.vapor_realign(realign.Options(), "key", driver, 1, 2)
    req = next(gen)
    assert isinstance(req, drivers.Window)
    req = gen.send([10])
    assert isinstance(req, drivers.Score) and req.ref_seq == "REF1"
    req = gen.send([0.25])
    assert req.ref_seq == "REF2"
    err = KeyError("invert_base")
    req = gen.throw(err)
    assert isinstance(req, drivers.Figure)
    req = gen.send(None)
    assert isinstance(req, drivers.Realign) and (req.ref_seq, req.alt_seq, req.reads) == ("REF1", "ALT1", [["r", 0, "q"]])
    assert req.name is None and req.options == realign.Options()
    with pytest.raises(StopIteration) as fin:
        gen.send(realign.Payload([12]))
    out = fin.value.value
    assert type(out) is drivers.Realigned and out == [0.5] and out.realign == [12] and seen == [[10], [0.25], err]
    # a driver that makes no Score request: no Realign request, no payload
    def none(_a):
        yield drivers.Window("W")
        return []
    gen = drivers.vapor_realign(realign.Options(), "key", none, 0)
    next(gen)
    with pytest.raises(StopIteration) as fin:
        gen.send([10])
    assert fin.value.value == [] and fin.value.value.realign is None
